"""CPU tests of the reference-frame capture's boundary (include/fdoct_capture.h): the exports, the function-try-block at
every entry point, the header as C99, fdoct_normalize_minmax against the oracle's cv::normalize bit for bit, and error codes
instead of crashes without a device or with bad arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import capture_model
import fdoct_amd
import oracle_lib
from fdoct_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EPS = float(np.finfo(np.float64).eps)


def _declared(header):
    return sorted(set(re.findall(r"\b(fdoct_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", header)).read())))


def test_capture_header_is_exported_and_listed_and_disjoint_from_the_other_headers():
    declared = _declared("fdoct_capture.h")
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(capi.CAPTURE_ABI_SYMBOLS) == declared and len(declared) == 4
    base = _declared("fdoct.h")
    assert sorted(capi.ABI_SYMBOLS) == base and len(base) == 50
    assert not set(declared) & set(base)
    assert not set(declared) & set(capi.ROI_ABI_SYMBOLS)
    assert sorted(capi.ROI_ABI_SYMBOLS) == _declared("fdoct_roi.h")


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


def test_every_capture_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_capture.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.CAPTURE_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"
    # the 50 of fdoct_capi.cpp are still the ABI of fdoct.h
    base = [d[0] for d in _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_capi.cpp"))]
    assert len(base) == 50 and set(base) == set(capi.ABI_SYMBOLS)


def test_capture_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_capture.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_capture.h"
int main(void) {
  double y[3] = {1.0, 2.0, 4.0};
  fdoct_ref_role r = FDOCT_REF_NONE;
  int (*cap)(fdoct_handle, int, const void*, fdoct_dtype, fdoct_memspace, int, size_t, double*) = fdoct_capture_reference;
  int (*get)(fdoct_handle, int, double*, size_t, int*) = fdoct_get_reference;
  int (*mm)(fdoct_handle, const void*, fdoct_dtype, fdoct_memspace, int, size_t, double*, double*, fdoct_memspace) = fdoct_frame_minmax;
  (void)cap; (void)get; (void)mm;
  return fdoct_normalize_minmax(y, 3, 0.0001, 1.0) + (r == 3 ? 0 : 1);
}
""")
    obj = tmp_path / "use_capture.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    assert obj.exists()


def _same_bits(got, want):
    assert np.array_equal(capture_model.bits(got), capture_model.bits(want))


def _normalize_cases():
    rng = np.random.default_rng(20)
    backg = np.fromfile(os.path.join(GOLD, "backg_u16_96x128.bin"), np.uint16).astype(np.float64)
    yield "golden backg", backg
    yield "random", rng.standard_normal(5000) * 1e3
    yield "random, small positive", rng.random(4097) * 1e-9
    yield "constant", np.full(77, 1234.5)
    yield "range just above DBL_EPSILON", np.array([1.0, 1.0 + 2 * EPS, 1.0 + EPS])
    yield "range exactly DBL_EPSILON (not above)", np.array([1.0, 1.0 + EPS])
    yield "range just below DBL_EPSILON", np.array([0.5, 0.5 + EPS / 2, 0.5])
    yield "n = 1", np.array([42.0])
    yield "negative and zero", np.array([-3.0, 0.0, -0.0, 7.5, -1e-300])


@pytest.mark.parametrize("lo,hi", [(0.0001, 1.0), (0.0, 1.0), (1.0, 0.0001), (-2.5, 17.0)])
def test_normalize_minmax_equals_the_oracle_bit_for_bit(lo, hi):
    for what, y in _normalize_cases():
        got = capi.normalize_minmax(y, lo, hi)
        want = oracle_lib.normalize_minmax(y, lo, hi)
        assert np.array_equal(capture_model.bits(got), capture_model.bits(want)), what
    # a constant array: scale 0, every element the lower limit
    assert np.all(capi.normalize_minmax(np.full(9, 3.25), lo, hi) == min(lo, hi))


def test_normalize_minmax_empty_and_null_return_codes():
    lib = fdoct_amd.load_library()
    y = np.array([1.0, 2.0])
    assert lib.fdoct_normalize_minmax(None, 0, 0.0, 1.0) == 0
    assert lib.fdoct_normalize_minmax(y.ctypes.data, 0, 0.0, 1.0) == 0 and y.tolist() == [1.0, 2.0]
    assert lib.fdoct_normalize_minmax(None, 4, 0.0, 1.0) == -1
    assert capi.normalize_minmax([], 0.0, 1.0).size == 0
    assert fdoct_amd.normalize_minmax is capi.normalize_minmax


def test_capture_model_composes_the_oracle_recipe():
    """The model on a case small enough to restate by hand: two frames, both normalisations, then the division branch."""
    f = np.array([[[1, 5, 9], [2, 2, 4]], [[3, 1, 1], [0, 6, 2]]], np.uint16)
    acc = np.array([[4.0, 6.0, 10.0], [2.0, 8.0, 6.0]])
    _same_bits(capture_model.capture(capture_model.BACKGROUND, f), acc / 2.0)
    rows = np.stack([oracle_lib.normalize_minmax(r, 0.0001, 1.0) for r in acc])
    _same_bits(capture_model.capture(capture_model.DARK, f, rowwisenormalize=1, donotnormalize=0),
               oracle_lib.normalize_minmax(rows.ravel(), 0.0001, 1.0).reshape(2, 3))
    _same_bits(capture_model.capture(capture_model.PI, f[:1], rowwisenormalize=0, donotnormalize=0),
               oracle_lib.normalize_minmax(f[0].astype(np.float64).ravel(), 0.0, 1.0).reshape(2, 3))
    _same_bits(capture_model.capture(capture_model.BACKGROUND, f[:1], donotnormalize=0, sim=True), f[0].astype(np.float64))
    # smoothmovavg before the accumulation (main:990-991, 1043)
    want = oracle_lib.smoothmovavg(f[0].astype(np.float64), 2) + oracle_lib.smoothmovavg(f[1].astype(np.float64), 2)
    _same_bits(capture_model.capture(capture_model.NONE, f, movavgn=2), want / 2.0)


def test_capture_entry_points_refuse_null_handles_and_bad_arguments_without_a_device():
    lib = fdoct_amd.load_library()
    buf = np.zeros(64, np.uint16)
    d = np.zeros(64, np.float64)
    rows = C.c_int()
    assert lib.fdoct_capture_reference(None, 0, buf.ctypes.data, 1, 0, 1, 0, d.ctypes.data) == -1
    assert lib.fdoct_get_reference(None, 0, d.ctypes.data, 64, C.byref(rows)) == -1
    assert lib.fdoct_frame_minmax(None, buf.ctypes.data, 1, 0, 1, 0, d.ctypes.data, d.ctypes.data, 0) == -1
    assert lib.fdoct_normalize_minmax(None, 1, 0.0, 1.0) == -1
    import torch
    if not torch.cuda.is_available():   # no handle can exist without a device: there is nothing to compute on
        with pytest.raises(fdoct_amd.FdoctError) as e:
            fdoct_amd.Reconstructor(fdoct_amd.Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128))
        assert e.value.code == -3
