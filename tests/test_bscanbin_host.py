"""CPU tests of the output binning's boundary (include/fdoct_bscanbin.h) on the built library, without a device: the tap table
against the model bit for bit, the result's size, error codes instead of crashes, and the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bscanbin_model as m
import fdoct_amd
from fdoct_amd import capi
from test_roi_host import _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


def test_bscanbin_header_is_exported_and_listed_and_on_its_own():
    hdr = open(os.path.join(ROOT, "include", "fdoct_bscanbin.h")).read()
    declared = sorted(set(re.findall(r"\b(fdoct_[a-z_0-9]+)\s*\(", hdr)))
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(capi.BSCANBIN_ABI_SYMBOLS) == declared and len(declared) == 3
    others = set(capi.ABI_SYMBOLS) | set(capi.ROI_ABI_SYMBOLS) | set(capi.CAPTURE_ABI_SYMBOLS) | set(capi.LOWPASS_ABI_SYMBOLS)
    assert not set(declared) & others
    base = open(os.path.join(ROOT, "include", "fdoct.h")).read()
    assert "bscanbin" not in base and "bscan_bin" not in base
    # what the library exports under the new names is exactly the list
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if re.search(r" T fdoct_bscan", ln)}
    assert exported == set(capi.BSCANBIN_ABI_SYMBOLS)


def test_every_bscanbin_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_bscanbin.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.BSCANBIN_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"
    base = [d[0] for d in _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_capi.cpp"))]
    assert not set(base) & set(names)


def test_taps_equal_the_models_truth_mode_bit_for_bit():
    for u in range(1, m.MAX_UP + 1):
        taps, off = capi.bscanbin_taps(u)
        want, want_off = m.taps(u, "truth")
        assert taps.tobytes() == want.tobytes(), u
        np.testing.assert_array_equal(off, want_off)
    assert capi.bscanbin_taps(1)[0].tolist() == [[0.0, 1.0, 0.0, 0.0]]
    lib = fdoct_amd.load_library()
    t = np.zeros(4 * 64)
    assert lib.fdoct_bscanbin_taps(3, t.ctypes.data, None) == 0          # the offsets are optional
    for up in (0, -1, 65):
        assert lib.fdoct_bscanbin_taps(up, t.ctypes.data, None) == INVALID
    assert lib.fdoct_bscanbin_taps(2, None, None) == INVALID


def test_size():
    assert capi.bscanbin_size(1024, 1000, 2, 2) == (1024, 1000)
    assert capi.bscanbin_size(1024, 1000, 2, 1, upx=4) == (1024, 2000)    # binvaluey = 2: upx = bscanbinx * binvaluey
    assert capi.bscanbin_size(96, 512, 1, 4) == (96, 512)
    assert capi.bscanbin_size(96, 512, 16, 16, 1, 1) == (6, 32)
    assert capi.bscanbin_size(15, 25, 5, 3, 64, 64) == (5 * 64, 5 * 64)
    for D, H, bx, by, ux, uy in [(1024, 1000, 3, 1, 3, 1), (1023, 1000, 1, 2, 1, 2), (10, 10, 16, 1, 1, 1)]:
        assert m.out_size(D, H, bx, by, ux, uy) is not None
        with pytest.raises(fdoct_amd.FdoctError) as e:
            capi.bscanbin_size(D, H, bx, by, ux, uy)
        assert e.value.code == UNSUPPORTED
    for D, H, bx, by, ux, uy in [(8, 8, 0, 1, 1, 1), (8, 8, 1, 17, 1, 1), (8, 8, 1, 1, 65, 1), (8, 8, 1, 1, 1, 0), (0, 8, 1, 1, 1, 1),
                                 (8, -4, 1, 1, 1, 1)]:
        with pytest.raises(fdoct_amd.FdoctError) as e:
            capi.bscanbin_size(D, H, bx, by, ux, uy)
        assert e.value.code == INVALID
    lib = fdoct_amd.load_library()
    n = C.c_int()
    assert lib.fdoct_bscanbin_size(8, 8, 2, 2, 2, 2, None, C.byref(n)) == INVALID
    assert lib.fdoct_bscanbin_size(8, 8, 2, 2, 2, 2, C.byref(n), None) == INVALID


def test_bscan_bin_refuses_bad_calls_without_a_device():
    """Arguments are judged before the handle is touched: the same refusals with and without a GPU."""
    lib = fdoct_amd.load_library()
    buf = np.zeros(3 * 64, np.float32)
    src, out, out2 = buf[:64].ctypes.data, buf[64:128].ctypes.data, buf[128:].ctypes.data

    def call(bscan=src, jscan=None, mem=0, layout=0, n=1, D=8, H=8, bx=2, by=2, ux=2, uy=2, mf=4.0, o=out, odb=out2, omem=0):
        return lib.fdoct_bscan_bin(None, bscan, jscan, mem, layout, n, D, H, bx, by, ux, uy, mf, o, odb, omem)

    assert call() == INVALID                                             # a null handle, everything else in order
    assert call(bscan=None) == INVALID and call(o=None, odb=None) == INVALID
    assert call(mem=2) == INVALID and call(omem=-1) == INVALID and call(layout=2) == INVALID and call(n=0) == INVALID
    assert call(bx=0) == INVALID and call(by=17) == INVALID and call(ux=65) == INVALID and call(uy=0) == INVALID
    assert call(mf=float("nan")) == INVALID and call(mf=float("inf")) == INVALID
    assert call(D=9) == UNSUPPORTED and call(H=7, bx=2) == UNSUPPORTED and call(D=8, by=3) == UNSUPPORTED
    assert b"multiple" in lib.fdoct_last_error(None)
    # overlapping buffers: output on input, the two outputs on each other, an output on jscan
    assert call(o=src) == INVALID and b"overlap" in lib.fdoct_last_error(None)
    assert call(o=src + 4 * 63) == INVALID and call(odb=out + 4) == INVALID and call(jscan=out2, odb=out2) == INVALID
    assert b"overlap" in lib.fdoct_last_error(None)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(fdoct_amd.FdoctError) as e:
            fdoct_amd.Reconstructor(fdoct_amd.Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128))
        assert e.value.code == -3
