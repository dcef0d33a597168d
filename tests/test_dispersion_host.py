"""CPU tests of the dispersion search's boundary (include/fdoct_dispersion.h): libfdoct_dispersion.so exports exactly the header's
symbols and the other four libraries none of them, the entry points are function-try-blocks, the header compiles as C99 next to
fdoct.h, a NULL handle is refused with the outputs untouched, fdoct_dispersion_plan holds on a table of cases with its refusals,
fdoct_dispersion_phase_table is within one float ulp of synth.dispersion_phase, and the binding checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dispersion_model as dm
import fdoct_amd
from fdoct_amd import capi, dispersion, synth
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A2, A3 = (-24.0, 4.0, 13), (-8.0, 2.0, 9)


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_dispersion_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_dispersion.h")
    assert declared == sorted(dispersion.DISPERSION_ABI_SYMBOLS) == ["fdoct_dispersion_phase_table", "fdoct_dispersion_plan", "fdoct_dispersion_search",
                                                                      "fdoct_process_dispersion_search"]
    assert _exports(dispersion.library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path(), capi.doppler_library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(dispersion.library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS +
              capi.DOPPLER_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    needed = subprocess.check_output(["readelf", "-d", dispersion.library_path()], text=True)
    assert "libfdoct_hip.so" in needed and "$ORIGIN" in needed
    # functions over a Reconstructor, not methods of it
    for name in ("library_path", "phase_table", "plan", "search", "search_device", "process_search", "process_search_device"):
        assert callable(getattr(dispersion, name)) and not hasattr(capi.Reconstructor, name)


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_dispersion.cpp"))
    assert [d[0] for d in defs] == dispersion.DISPERSION_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_dispersion_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_dispersion.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_dispersion.h"
int main(void) {
  float x[64], table[32], out[4] = {7.f, 7.f, 7.f, 7.f};
  double sums[2] = {7.0, 7.0};
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_dispersion_grid g = {-24.0, 4.0, 13, -8.0, 2.0, 9, 2, 0};
  fdoct_dispersion_info info;
  fdoct_dispersion_best best = {5, 5, 5, 5.0, 5.0, 5.0};
  int i;
  for (i = 0; i < 64; i++) x[i] = 1.f;
  if (fdoct_dispersion_plan(&g, 3, 96, &info) != FDOCT_OK || info.candidates != 117 || info.per_workgroup != 8 || info.chunks != 15 ||
      info.workgroups != 45 || info.lds_bytes < 3u * 96u * 8u) return 1;
  info.candidates = -3;
  if (fdoct_dispersion_plan(&g, 3, 97, &info) != FDOCT_ERR_UNSUPPORTED || info.candidates != -3) return 2;
  if (fdoct_dispersion_plan(&g, 3, 8, &info) != FDOCT_ERR_INVALID || info.candidates != -3) return 3;
  if (fdoct_dispersion_phase_table(16, 0.0, 0.0, table) != FDOCT_OK || table[0] != 1.f || table[1] != 0.f || table[31] != 0.f) return 4;
  if (fdoct_dispersion_search(NULL, x, FDOCT_MEM_HOST, 2, 16, &g, sums, NULL, &best, out, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 5;
  if (fdoct_process_dispersion_search(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 1, 0, &g, sums, NULL, &best, out, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID)
    return 6;
  return (out[0] == 7.f && out[3] == 7.f && sums[0] == 7.0 && best.index == 5 && best.metric == 5.0) ? 0 : 7;
}
""")
    exe = tmp_path / "use_dispersion"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_dispersion", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    X = np.full(2 * 16, 2 + 1j, np.complex64)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(4096, -7.0, np.float64) for _ in range(4)]
    g = dispersion.grid(A2, A3, (2, 0))
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_dispersion_search(None, X.ctypes.data, space, 2, 16, g, *ptrs, space) == -1
        assert lib.fdoct_process_dispersion_search(None, frames.ctypes.data, capi.DTYPE_U16, space, 1, 0, g, *ptrs, space) == -1
    assert lib.fdoct_dispersion_search(None, None, 0, 2, 16, None, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(X == np.complex64(2 + 1j))
    assert C.sizeof(dispersion._CGrid) == 56 and C.sizeof(dispersion._CBest) == 40 == dispersion.BEST_DTYPE.itemsize and C.sizeof(dispersion._CInfo) == 32


def _lds(n):
    return 3 * n * 8 + 2 * 4 * 8


# (a2, a3, rows, n, depth) -> (candidates, per_workgroup, chunks, workgroups), or the refusal's code
PLAN_CASES = [
    ((A2, A3, 3, 96, (2, 0)), (117, 8, 15, 45)),
    ((A2, A3, 1, 4096, (2, 0)), (117, 8, 15, 15)),
    ((A2, A3, 1, 16, (0, 0)), (117, 8, 15, 15)),
    ((A2, A3, 64, 2048, (2, 0)), (117, 8, 15, 960)),                          # rows K = 7488: still the floor of 8
    ((A2, A3, 256, 2048, (2, 0)), (117, 8, 15, 3840)),
    ((A2, A3, 1024, 2048, (2, 0)), (117, 15, 8, 8192)),                       # ceil(119808 / 8192) = 15
    (((0.0, 1.0, 64), (0.0, 1.0, 64), 64, 2048, (0, 0)), (4096, 32, 128, 8192)),   # a 64 x 64 grid over 64 A-scans
    (((0.0, 1.0, 5), (0.0, 1.0, 3), 2, 128, (0, 0)), (15, 8, 2, 4)),         # two chunks, the second of 7
    (((8.0, 0.0, 1), (-2.0, 0.0, 1), 2, 96, (0, 0)), (1, 1, 1, 2)),          # one candidate: the chunk is capped at K
    (((0.0, 1.0, 3), (0.0, 1.0, 2), 5, 160, (0, 0)), (6, 6, 1, 5)),
    (((0.0, 1.0, 256), (0.0, 1.0, 256), 256, 1024, (0, 0)), (65536, 2048, 32, 8192)),   # both bounds met: K = 65536, rows K = 2^24
    (((0.0, 1.0, 256), (0.0, 1.0, 256), 257, 1024, (0, 0)), -1),             # rows K beyond 2^24
    (((0.0, 1.0, 257), (0.0, 1.0, 256), 1, 1024, (0, 0)), -1),               # K beyond 65536
    (((0.0, 1.0, 65536), (0.0, 1.0, 65536), 1, 1024, (0, 0)), -1),           # (a product that would wrap an int)
    (((0.0, 1.0, 0), A3, 1, 128, (0, 0)), -1), ((A2, (0.0, 1.0, 0), 1, 128, (0, 0)), -1), (((0.0, 1.0, -1), A3, 1, 128, (0, 0)), -1),
    ((A2, A3, 0, 128, (0, 0)), -1), ((A2, A3, -1, 128, (0, 0)), -1),
    ((A2, A3, 1, 15, (0, 0)), -1), ((A2, A3, 1, 8, (0, 0)), -1), ((A2, A3, 1, 0, (0, 0)), -1), ((A2, A3, 1, -16, (0, 0)), -1),
    ((A2, A3, 1, 4097, (0, 0)), -2), ((A2, A3, 1, 8192, (0, 0)), -2), ((A2, A3, 1, 4100, (0, 0)), -2),   # longer rows
    ((A2, A3, 1, 17, (0, 0)), -2), ((A2, A3, 1, 112, (0, 0)), -2), ((A2, A3, 1, 4094, (0, 0)), -2),      # a prime factor above 5
    ((A2, A3, 1, 4050, (0, 0)), (117, 8, 15, 15)), ((A2, A3, 1, 3125, (0, 0)), (117, 8, 15, 15)), ((A2, A3, 1, 2187, (0, 0)), (117, 8, 15, 15)),
    ((A2, A3, 1, 18, (0, 0)), (117, 8, 15, 15)), ((A2, A3, 1, 25, (0, 0)), (117, 8, 15, 15)),
    (((float("nan"), 4.0, 13), A3, 1, 128, (0, 0)), -1), (((-24.0, float("inf"), 13), A3, 1, 128, (0, 0)), -1),
    ((A2, (float("-inf"), 2.0, 9), 1, 128, (0, 0)), -1), ((A2, (-8.0, float("nan"), 9), 1, 128, (0, 0)), -1),
    ((A2, A3, 1, 128, (0, 128)), (117, 8, 15, 15)), ((A2, A3, 1, 128, (127, 1)), (117, 8, 15, 15)), ((A2, A3, 1, 128, (63, 0)), (117, 8, 15, 15)),
    ((A2, A3, 1, 128, (64, 0)), -1),                                          # up to n / 2 from n / 2: no bin
    ((A2, A3, 1, 128, (100, 0)), -1), ((A2, A3, 1, 128, (128, 0)), -1), ((A2, A3, 1, 128, (128, 1)), -1), ((A2, A3, 1, 128, (-1, 4)), -1),
    ((A2, A3, 1, 128, (0, 129)), -1), ((A2, A3, 1, 128, (127, 2)), -1), ((A2, A3, 1, 128, (0, -1)), -1),
]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[str(c[0]) for c in PLAN_CASES])
def test_dispersion_plan(case):
    (a2, a3, rows, n, depth), want = case
    if isinstance(want, int):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            dispersion.plan(a2, a3, rows, n, depth)
        assert e.value.code == want
    else:
        p = dispersion.plan(a2, a3, rows, n, depth)
        assert (p["candidates"], p["per_workgroup"], p["chunks"], p["workgroups"]) == want
        assert p["lds_bytes"] == _lds(n) <= 160 * 1024
        K = want[0]
        assert p["workspace_bytes"] == (1 + a2[2] + a3[2]) * n * 8 + rows * K * 16 + K * 16 + n * 8 + 40


def test_dispersion_plan_refuses_missing_pointers_and_leaves_its_output_alone():
    lib = fdoct_amd.load_library()
    g, info = dispersion.grid(A2, A3), dispersion._CInfo(-5, -6, -7, 8, -9, 10)
    assert lib.fdoct_dispersion_plan(None, 1, 128, C.byref(info)) == -1
    assert lib.fdoct_dispersion_plan(C.byref(g), 1, 128, None) == -1
    assert lib.fdoct_dispersion_plan(C.byref(g), 1, 17, C.byref(info)) == -2
    assert (info.candidates, info.per_workgroup, info.chunks, info.lds_bytes, info.workgroups, info.workspace_bytes) == (-5, -6, -7, 8, -9, 10)


@pytest.mark.parametrize("n,a2,a3", [(16, 0.0, 0.0), (96, 8.0, -2.0), (2048, 20.0, 5.0), (4096, -24.0, 8.0), (75, 3.25, -1.5), (1, 1.0, 1.0), (5000, 12.0, -4.0)])
def test_phase_table_is_within_one_float_ulp_of_synth(n, a2, a3):
    got = dispersion.phase_table(n, a2, a3)
    assert got.shape == (n, 2) and got.dtype == np.float32
    assert dm.ulp_apart(got, synth.dispersion_phase(n, a2, a3)) <= 1.0
    assert dm.ulp_apart(got, dm.phase_table(n, a2, a3)) <= 1.0
    np.testing.assert_allclose(np.hypot(got[:, 0], got[:, 1]), 1.0, atol=2e-7)


def test_phase_table_refusals_leave_the_output_alone():
    lib = fdoct_amd.load_library()
    out = np.full(32, -7.0, np.float32)
    for n, a2, a3, p in ((0, 1.0, 1.0, out.ctypes.data), (-4, 1.0, 1.0, out.ctypes.data), (16, float("nan"), 1.0, out.ctypes.data),
                         (16, 1.0, float("inf"), out.ctypes.data), (16, 1.0, 1.0, None)):
        assert lib.fdoct_dispersion_phase_table(n, a2, a3, p) == -1
    assert np.all(out == -7.0)
    with pytest.raises(fdoct_amd.FdoctError):
        dispersion.phase_table(0, 1.0, 1.0)


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=128, numdisplaypoints=128)
    X = np.zeros((4, 128), np.complex64)
    for bad in (X.astype(np.complex128), X.view(np.float32), np.zeros((4, 128), np.float32), np.zeros((0, 128), np.complex64)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            dispersion.search(rec, bad, A2, A3)
        assert e.value.code == -1 and "complex64" in str(e.value)
    for kw in (dict(want=()), dict(want=("sums", "metric")), dict(want=("best", "best")), dict(want="table"), dict(a2=3.0), dict(a2=(1.0, 2.0)),
               dict(a3=(0.0, 1.0, "x")), dict(depth=5), dict(depth=(1, 2, 3)), dict(a2=(0.0, 1.0, 0)), dict(a3=(float("nan"), 1.0, 3)),
               dict(depth=(128, 0)), dict(depth=(0, 129))):
        args = dict(dict(a2=A2, a3=A3), **kw)
        with pytest.raises(fdoct_amd.FdoctError) as e:
            dispersion.search(rec, X, **args)
        assert e.value.code == -1, kw
    with pytest.raises(fdoct_amd.FdoctError) as e:
        dispersion.search(rec, np.zeros((2, 112), np.complex64), A2, A3)     # 112 = 16 x 7
    assert e.value.code == -2
    frames = np.zeros((2, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        dispersion.process_search(rec, frames.astype(np.int64), A2, A3)
    assert e.value.code == -1 and "dtype" in str(e.value)
    short = capi.Reconstructor.__new__(capi.Reconstructor)
    short.lib, short.h, short.cfg = rec.lib, None, fdoct_amd.Config(width=8, height=4, numfftpoints=128, numdisplaypoints=64)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        dispersion.process_search(short, frames, A2, A3)
    assert e.value.code == -2 and "numdisplaypoints" in str(e.value)
    for call in (lambda: dispersion.search(rec, X, A2, A3, want="sums"), lambda: dispersion.process_search(rec, frames, A2, A3, depth=(2, 0)),
                 lambda: dispersion.search_device(rec, 4096, 4, 128, A2, A3, 8192, None, None, None),
                 lambda: dispersion.process_search_device(rec, 4096, capi.DTYPE_U16, 2, 16, A2, A3, None, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = short.h = None
