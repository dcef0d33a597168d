"""CPU tests of the Doppler stage's boundary (include/fdoct_doppler.h): libfdoct_doppler.so exports exactly the header's symbols and
the other three libraries none of them, the entry points are function-try-blocks, the header compiles as C99 next to fdoct.h, a
NULL handle is refused with the outputs untouched, fdoct_doppler_size holds on a table of cases with its refusals, and the binding
checks its arguments."""
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, F = capi.DOPPLER_ASCANS, capi.DOPPLER_FRAMES


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_doppler_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_doppler.h")
    assert declared == sorted(capi.DOPPLER_ABI_SYMBOLS) == ["fdoct_doppler", "fdoct_doppler_size", "fdoct_process_doppler"]
    assert _exports(capi.doppler_library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(capi.doppler_library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    assert _declared("fdoct_complex.h") == sorted(capi.COMPLEX_ABI_SYMBOLS)   # the complex header is what it was
    needed = subprocess.check_output(["readelf", "-d", capi.doppler_library_path()], text=True)
    assert "libfdoct_hip.so" in needed and "$ORIGIN" in needed


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_doppler.cpp"))
    assert [d[0] for d in defs] == capi.DOPPLER_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_doppler_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_doppler.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_doppler.h"
int main(void) {
  float x[8] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f}, out[4] = {7.f, 7.f, 7.f, 7.f};
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_doppler_params p = {FDOCT_DOPPLER_ASCANS, 1, 3, 5, 0, 0, 0, 1.0, 0.0};
  int images = -1, rows = -1;
  if (fdoct_doppler_size(&p, 2, 12, 20, &images, &rows) != FDOCT_OK || images != 2 || rows != 11) return 1;
  p.axis = FDOCT_DOPPLER_FRAMES;
  if (fdoct_doppler_size(&p, 3, 12, 20, &images, &rows) != FDOCT_OK || images != 2 || rows != 12) return 2;
  p.win_depths = 33;
  if (fdoct_doppler_size(&p, 3, 12, 20, &images, &rows) != FDOCT_ERR_INVALID || images != 2 || rows != 12) return 3;
  if (fdoct_doppler(NULL, x, FDOCT_MEM_HOST, 1, 2, 2, &p, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 4;
  if (fdoct_process_doppler(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 1, 0, &p, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 5;
  return (out[0] == 7.f && out[3] == 7.f) ? 0 : 6;
}
""")
    exe = tmp_path / "use_doppler"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_doppler", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    X = np.full(2 * 3 * 4, 2 + 1j, np.complex64)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(64, -7.0, np.float32) for _ in range(3)]
    p = capi.doppler_params(A, 1, (3, 5))
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_doppler(None, X.ctypes.data, space, 2, 3, 4, p, *ptrs, space) == -1
        assert lib.fdoct_process_doppler(None, frames.ctypes.data, capi.DTYPE_U16, space, 1, 0, p, *ptrs, space) == -1
    assert lib.fdoct_doppler(None, None, 0, 2, 3, 4, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(X == np.complex64(2 + 1j))


# (axis, lag, nframes, ascans, depths, keywords) -> (pair_images, pair_rows), or None where the call is refused
SIZE_CASES = [
    ((A, 1, 1, 2, 1, {}), (1, 1)),
    ((A, 1, 2, 12, 20, {}), (2, 11)),
    ((A, 11, 2, 12, 20, {}), (2, 1)),
    ((A, 12, 2, 12, 20, {}), None),                               # no pair row left
    ((A, 1, 5, 1, 20, {}), None),
    ((F, 1, 2, 12, 20, {}), (1, 12)),
    ((F, 2, 5, 1000, 1024, dict(win=(4, 8))), (3, 1000)),
    ((F, 2, 2, 12, 20, {}), None),                                # no pair image left
    ((F, 1, 1, 12, 20, {}), None),
    ((A, 0, 2, 12, 20, {}), None), ((A, -1, 2, 12, 20, {}), None),
    ((2, 1, 2, 12, 20, {}), None), ((-1, 1, 2, 12, 20, {}), None),
    ((A, 1, 0, 12, 20, {}), None), ((A, 1, 2, 0, 20, {}), None), ((A, 1, 2, 12, 0, {}), None),
    ((A, 1, 2, 12, 20, dict(win=(32, 32))), (2, 11)),
    ((A, 1, 2, 12, 20, dict(win=(33, 1))), None), ((A, 1, 2, 12, 20, dict(win=(1, 33))), None),
    ((A, 1, 2, 12, 20, dict(win=(0, 1))), None), ((A, 1, 2, 12, 20, dict(win=(1, 0))), None), ((A, 1, 2, 12, 20, dict(win=(-3, 5))), None),
    ((A, 1, 2, 12, 20, dict(bulk=True)), (2, 11)),
    ((A, 1, 2, 12, 20, dict(bulk=(19, 1))), (2, 11)), ((A, 1, 2, 12, 20, dict(bulk=(19, 0))), (2, 11)), ((A, 1, 2, 12, 20, dict(bulk=(0, 20))), (2, 11)),
    ((A, 1, 2, 12, 20, dict(bulk=(20, 0))), None), ((A, 1, 2, 12, 20, dict(bulk=(19, 2))), None), ((A, 1, 2, 12, 20, dict(bulk=(-1, 2))), None),
    ((A, 1, 2, 12, 20, dict(bulk=(0, -1))), None), ((A, 1, 2, 12, 20, dict(bulk=(0, 21))), None),
    ((A, 1, 2, 12, 20, dict(scale=-3.5, min_power=0.0)), (2, 11)), ((A, 1, 2, 12, 20, dict(scale=0.0, min_power=1e30)), (2, 11)),
    ((A, 1, 2, 12, 20, dict(scale=float("nan"))), None), ((A, 1, 2, 12, 20, dict(scale=float("-inf"))), None),
    ((A, 1, 2, 12, 20, dict(min_power=float("nan"))), None), ((A, 1, 2, 12, 20, dict(min_power=float("inf"))), None),
    ((A, 1, 2, 12, 20, dict(min_power=-1e-30)), None),
    ((A, 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, {}), (2 ** 31 - 1, 2 ** 31 - 2)),   # the shape alone: sizes are the entry points' to refuse
]


@pytest.mark.parametrize("case", SIZE_CASES, ids=[str(c[0]) for c in SIZE_CASES])
def test_doppler_size(case):
    (axis, lag, n, h, d, kw), want = case
    if want is None:
        with pytest.raises(fdoct_amd.FdoctError) as e:
            capi.doppler_size(axis, lag, n, h, d, **kw)
        assert e.value.code == -1
    else:
        assert capi.doppler_size(axis, lag, n, h, d, **kw) == want


def test_doppler_size_refuses_missing_pointers_and_leaves_its_outputs_alone():
    import ctypes as C
    lib = fdoct_amd.load_library()
    p = capi.doppler_params(A, 1)
    a, b = C.c_int(-5), C.c_int(-6)
    assert lib.fdoct_doppler_size(None, 2, 12, 20, C.byref(a), C.byref(b)) == -1
    assert lib.fdoct_doppler_size(p, 2, 12, 20, None, C.byref(b)) == -1 and lib.fdoct_doppler_size(p, 2, 12, 20, C.byref(a), None) == -1
    bad = capi.doppler_params(A, 12)
    assert lib.fdoct_doppler_size(bad, 2, 12, 20, C.byref(a), C.byref(b)) == -1
    assert (a.value, b.value) == (-5, -6)
    assert C.sizeof(capi._CDopplerParams) == 48   # seven ints, padding to the doubles' alignment, two doubles


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=256, numdisplaypoints=128)
    X = np.zeros((2, 4, 16), np.complex64)
    for bad in (X.astype(np.complex128), X.view(np.float32), X[0], np.zeros((2, 4, 16), np.float32)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.doppler(bad, A, 1)
        assert e.value.code == -1 and "complex64" in str(e.value)
    for kw in (dict(want=()), dict(want=("phase", "angle")), dict(want=("corr", "corr")), dict(want="velocity"), dict(win=3), dict(win=(1, 2, 3)),
               dict(bulk=5), dict(bulk=(1, 2, 3)), dict(win=(0, 1)), dict(lag=4), dict(bulk=(16, 0)), dict(scale=float("nan")), dict(min_power=-1.0)):
        args = dict(dict(axis=A, lag=1), **kw)
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.doppler(X, **args)
        assert e.value.code == -1, kw
    frames = np.zeros((2, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        rec.process_doppler(frames.astype(np.int64), A, 1)
    assert e.value.code == -1 and "dtype" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        rec.process_doppler(frames, A, 4)          # height 4: no pair row left
    assert e.value.code == -1
    for call in (lambda: rec.doppler(X, A, 1, want="phase"), lambda: rec.process_doppler(frames, F, 1, win=(3, 5)),
                 lambda: rec.doppler_device(4096, 2, 4, 16, A, 1, 8192, None, None),
                 lambda: rec.process_doppler_device(4096, capi.DTYPE_U16, 2, 16, A, 1, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = None
