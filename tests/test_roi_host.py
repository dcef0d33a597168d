"""CPU tests of the B-scan readouts' boundary (include/fdoct_roi.h): the exports, the function-try-block at every entry point,
the besseldbinverse table edge by edge, and error codes instead of crashes without a device or with bad arguments."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fdoct_amd
import roi_model
from fdoct_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_roi_header_is_exported_and_listed_and_fdoct_h_is_unchanged():
    hdr = open(os.path.join(ROOT, "include", "fdoct_roi.h")).read()
    declared = sorted(set(re.findall(r"\b(fdoct_[a-z_0-9]+)\s*\(", hdr)))
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(capi.ROI_ABI_SYMBOLS) == declared
    base = sorted(set(re.findall(r"\b(fdoct_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "fdoct.h")).read())))
    assert sorted(capi.ABI_SYMBOLS) == base and len(base) == 50
    assert not set(declared) & set(base)


def _definitions(path):
    """(name, head, tail) of every extern "C" definition in a C-ABI source: what follows its closing brace."""
    src = open(path).read()
    body = src[src.index('extern "C" {'):src.rindex('}  // extern "C"')]

    def close_of(i):
        depth = 0
        while True:
            if body.startswith("//", i):
                i = body.index("\n", i)
                continue
            c = body[i]
            if c in "\"'":
                j = i + 1
                while body[j] != c:
                    j += 2 if body[j] == "\\" else 1
                i = j + 1
                continue
            depth += {"{": 1, "}": -1}.get(c, 0)
            if depth == 0:
                return i
            i += 1

    out = []
    for m in re.finditer(r"^(?!static\b)[A-Za-z_][\w \*]*?\b(fdoct_\w+)\(", body, re.M):
        head_end = min(k for k in (body.find("{", m.end()), body.find(";", m.end())) if k >= 0)
        if body[head_end] == ";":
            continue
        out.append((m.group(1), body[m.start():head_end], body[close_of(head_end) + 1:]))
    return out


def test_every_roi_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_roi.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.ROI_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"
    # the 50 of fdoct_capi.cpp are still the ABI of fdoct.h
    base = [d[0] for d in _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_capi.cpp"))]
    assert len(base) == 50 and set(base) == set(capi.ABI_SYMBOLS)


def test_besseldb_inverse_table_edges():
    t = np.array(roi_model.BINV_T)
    x = np.array(roi_model.BINV_X)
    assert len(t) == len(x) == 47 and np.all(np.diff(t) < 0) and np.all(np.diff(x) < 0)
    above = capi.besseldb_inverse(np.nextafter(t, np.inf))
    np.testing.assert_array_equal(above, x)                             # y just above t_i: x_i (comparison `>`)
    at = capi.besseldb_inverse(t)
    np.testing.assert_array_equal(at, np.append(x[1:], 0.0))           # y == t_i: the next lower output
    np.testing.assert_array_equal(capi.besseldb_inverse([0.0, -5.0, 1e9]), [0.0, 0.0, 2.38])
    # against the model, on a dense grid
    ys = np.linspace(-1, 35, 20001)
    np.testing.assert_array_equal(capi.besseldb_inverse(ys), [roi_model.besseldbinverse(v) for v in ys])


def test_besseldb_inverse_thresholds_follow_j0_below_the_top_three():
    """A typo guard: each threshold is |20 log10 J0(x - 0.02)| of its output x to 1 %; the top three entries (2.27, 2.33,
    2.38 above 21.65, 25, 30 dB) do not follow that rule in the reference and are pinned by the table test only."""
    from scipy.special import j0
    for t, x in list(zip(roi_model.BINV_T, roi_model.BINV_X))[3:]:
        want = abs(20 * math.log10(j0(x - 0.02)))
        assert abs(t - want) <= 0.01 * want, (t, x, want)


def test_roi_entry_points_refuse_null_handles_and_bad_arguments_without_a_device():
    lib = fdoct_amd.load_library()
    buf = np.zeros(64, np.float32)
    d = np.zeros(4, np.float64)
    f = np.zeros(4, np.float32)
    n = C.c_longlong()
    assert lib.fdoct_ascan_minmax(None, buf.ctypes.data, 0, 0, 1, 8, 8, 0, f.ctypes.data, f.ctypes.data, 0) == -1
    assert lib.fdoct_roi_mean(None, buf.ctypes.data, 0, 0, 1, 8, 8, 0, 0, 2, d.ctypes.data, 0) == -1
    assert lib.fdoct_set_peakhold_roi(None, 0, 0, 1, 1, 0) == -1
    assert lib.fdoct_peakhold(None, 1, buf.ctypes.data, 0, 0, 1, 8, 8) == -1
    assert lib.fdoct_get_peakhold(None, 1, f.ctypes.data, f.ctypes.data, C.byref(n)) == -1
    assert lib.fdoct_clear_peakhold(None, 1) == -1
    assert lib.fdoct_vibration_profile(None, 3, 0.0, d.ctypes.data, d.ctypes.data, d.ctypes.data) == -1
    assert lib.fdoct_besseldb_inverse(None, 4, d.ctypes.data) == -1
    assert lib.fdoct_besseldb_inverse(d.ctypes.data, -1, d.ctypes.data) == -1
    assert lib.fdoct_besseldb_inverse(None, 0, None) == 0
    import torch
    if not torch.cuda.is_available():   # no handle can exist without a device: there is nothing to compute on
        with pytest.raises(fdoct_amd.FdoctError) as e:
            fdoct_amd.Reconstructor(fdoct_amd.Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128))
        assert e.value.code == -3
