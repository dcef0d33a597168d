"""CPU tests of the angiography stage's boundary (include/fdoct_angio.h): libfdoct_angio.so exports exactly the header's symbols and
the other six libraries none of them, it needs libfdoct_hip.so and finds it through $ORIGIN, the entry points are
function-try-blocks, the header compiles as C99 next to fdoct.h, the ctypes mirrors have the structs' layout, a NULL handle is
refused with the outputs untouched, fdoct_angio_plan gives every refusal of the header's list that its arguments can show (the
pointers', memory spaces' and overlaps' need a call: tests/test_gpu_angio.py) with no GPU, and the binding checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
from fdoct_amd import angiography, capi, dispersion, vibrometry
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_angio_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_angio.h")
    assert declared == sorted(angiography.ANGIO_ABI_SYMBOLS) == ["fdoct_angio", "fdoct_angio_plan", "fdoct_process_angio"]
    assert _exports(angiography.library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path(), capi.doppler_library_path(),
                  dispersion.library_path(), vibrometry.library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(angiography.library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS +
              capi.DOPPLER_ABI_SYMBOLS + dispersion.DISPERSION_ABI_SYMBOLS + vibrometry.VIBRO_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    needed = subprocess.check_output(["readelf", "-d", angiography.library_path()], text=True)
    assert "libfdoct_hip.so" in needed and "$ORIGIN" in needed
    # functions over a Reconstructor, not methods of it
    for name in ("library_path", "params", "plan", "angio", "angio_device", "process_angio", "process_angio_device", "attach"):
        assert callable(getattr(angiography, name)) and not hasattr(capi.Reconstructor, name)


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_angio.cpp"))
    assert [d[0] for d in defs] == angiography.ANGIO_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_angio_header_compiles_as_c99_and_the_mirrors_have_its_layout(tmp_path):
    src = tmp_path / "use_angio.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "fdoct.h"
#include "fdoct_angio.h"
int main(void) {
  float x[2 * 6 * 3 * 5], out[4] = {7.f, 7.f, 7.f, 7.f};
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_angio_params p = {3, 3, 5, 1, 1, 2, 0.0};
  fdoct_angio_info info;
  int i;
  for (i = 0; i < 180; i++) x[i] = 1.f;
  if (fdoct_angio_plan(&p, 6, 3, 5, &info) != FDOCT_OK || info.groups != 2 || info.tiles != 2 || info.workgroups != 2) return 1;
  if (info.workspace_bytes != 2 * 2 * 3 * 8) return 2;
  info.groups = -3;
  p.repeats = 4;
  if (fdoct_angio_plan(&p, 6, 3, 5, &info) != FDOCT_ERR_INVALID || info.groups != -3) return 3;
  p.repeats = 3;
  if (fdoct_angio(NULL, x, FDOCT_MEM_HOST, 6, 3, 5, &p, NULL, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 4;
  if (fdoct_process_angio(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 2, 0, &p, NULL, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 5;
  if (out[0] != 7.f || out[3] != 7.f) return 6;
  printf("%d %d %d %d %d %d %d %d %d %d", (int)sizeof(fdoct_angio_params), (int)offsetof(fdoct_angio_params, win_depths),
         (int)offsetof(fdoct_angio_params, bulk_count), (int)offsetof(fdoct_angio_params, min_power), (int)sizeof(fdoct_angio_info),
         (int)offsetof(fdoct_angio_info, tiles), (int)offsetof(fdoct_angio_info, workgroups), (int)offsetof(fdoct_angio_info, workspace_bytes),
         FDOCT_ANGIO_MAX_WIN, FDOCT_ANGIO_MAX_REPEATS);
  return 0;
}
""")
    exe = tmp_path / "use_angio"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_angio", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    done = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.returncode
    P, I = angiography._CParams, angiography._CInfo
    assert [int(v) for v in done.stdout.split()] == [C.sizeof(P), P.win_depths.offset, P.bulk_count.offset, P.min_power.offset, C.sizeof(I), I.tiles.offset,
                                                     I.workgroups.offset, I.workspace_bytes.offset, angiography.MAX_WIN, angiography.MAX_REPEATS]
    assert C.sizeof(P) == 32 and C.sizeof(I) == 32


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    X = np.full(4 * 3 * 5, 2 + 1j, np.complex64)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(256, -7.0, np.float32) for _ in range(4)]
    p = angiography.params(repeats=2, bulk=True)
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_angio(None, X.ctypes.data, space, 4, 3, 5, p, *ptrs, space) == -1
        assert lib.fdoct_process_angio(None, frames.ctypes.data, capi.DTYPE_U16, space, 2, 0, p, *ptrs, space) == -1
    assert lib.fdoct_angio(None, None, 0, 4, 3, 5, None, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(X == np.complex64(2 + 1j))


GOOD = dict(repeats=3, win=(3, 5), bulk=(2, 3))
# (params' keywords, nframes, H, D) -> (groups, tiles, workgroups, workspace_bytes), or the refusal's code
PLAN_CASES = [
    ((GOOD, 6, 3, 20), (2, 2, 2, 2 * 2 * 3 * 8)), ((GOOD, 3, 17, 65), (1, 4, 4, 2 * 17 * 8)), ((dict(GOOD, bulk=None), 3, 17, 65), (1, 4, 4, 0)),
    ((dict(GOOD, repeats=2), 65536, 1, 20), (32768, 32768, 1024, 32768 * 8)), ((dict(GOOD, repeats=64), 64, 3, 20), (1, 1, 1, 63 * 3 * 8)),
    ((dict(GOOD, repeats=2), 2, 1 << 12, 1 << 12), (1, 256 * 64, 1024, (1 << 12) * 8)),                    # 2^24 pixels
    # repeats outside 2..64
    ((dict(GOOD, repeats=1), 6, 3, 20), -1), ((dict(GOOD, repeats=0), 6, 3, 20), -1), ((dict(GOOD, repeats=-2), 6, 3, 20), -1),
    ((dict(GOOD, repeats=65), 130, 3, 20), -1),
    # nframes not a positive multiple of repeats, or above 65536
    ((GOOD, 7, 3, 20), -1), ((GOOD, 2, 3, 20), -1), ((GOOD, 0, 3, 20), -1), ((GOOD, -3, 3, 20), -1), ((GOOD, 65538, 3, 20), -1),
    ((dict(GOOD, repeats=2), 65538, 3, 20), -1),
    # ascans or depths below 1, or their product above 2^24
    ((GOOD, 6, 0, 20), -1), ((GOOD, 6, 3, 0), -1), ((GOOD, 6, -3, 20), -1), ((GOOD, 6, 3, -20), -1), ((GOOD, 6, 1 << 12, (1 << 12) + 1), -1),
    ((GOOD, 6, 1 << 24, 5), -1), ((GOOD, 6, 1 << 16, 1 << 16), -1),
    # a window size outside 1..16
    ((dict(GOOD, win=(0, 5)), 6, 3, 20), -1), ((dict(GOOD, win=(3, 0)), 6, 3, 20), -1), ((dict(GOOD, win=(17, 5)), 6, 3, 20), -1),
    ((dict(GOOD, win=(3, 17)), 6, 3, 20), -1), ((dict(GOOD, win=(-1, 1)), 6, 3, 20), -1), ((dict(GOOD, win=(16, 16)), 6, 3, 20), (2, 2, 2, 96)),
    ((dict(GOOD, win=(1, 1)), 6, 3, 20), (2, 2, 2, 96)),
    # a bulk range outside [0, depths)
    ((dict(GOOD, bulk=(0, 0)), 6, 3, 20), (2, 2, 2, 96)), ((dict(GOOD, bulk=(19, 1)), 6, 3, 20), (2, 2, 2, 96)), ((dict(GOOD, bulk=(0, 20)), 6, 3, 20), (2, 2, 2, 96)),
    ((dict(GOOD, bulk=(20, 0)), 6, 3, 20), -1), ((dict(GOOD, bulk=(-1, 0)), 6, 3, 20), -1), ((dict(GOOD, bulk=(0, 21)), 6, 3, 20), -1),
    ((dict(GOOD, bulk=(19, 2)), 6, 3, 20), -1), ((dict(GOOD, bulk=(5, -1)), 6, 3, 20), -1),
    # min_power not finite or negative
    ((dict(GOOD, min_power=float("nan")), 6, 3, 20), -1), ((dict(GOOD, min_power=float("inf")), 6, 3, 20), -1), ((dict(GOOD, min_power=-1e-30), 6, 3, 20), -1),
    ((dict(GOOD, min_power=2.5), 6, 3, 20), (2, 2, 2, 96)),
]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[str(c[0]) for c in PLAN_CASES])
def test_angio_plan(case):
    (kw, T, H, D), want = case
    if isinstance(want, int):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            angiography.plan(kw, T, H, D)
        assert e.value.code == want
    else:
        p = angiography.plan(kw, T, H, D)
        assert (p["groups"], p["tiles"], p["workgroups"], p["workspace_bytes"]) == want


def test_angio_plan_refuses_missing_pointers_and_a_bad_bulk_flag_and_leaves_its_output_alone():
    lib = fdoct_amd.load_library()
    p, info = angiography.params(**GOOD), angiography._CInfo(-5, -6, -7, 8)
    assert lib.fdoct_angio_plan(None, 6, 3, 20, C.byref(info)) == -1
    assert lib.fdoct_angio_plan(C.byref(p), 6, 3, 20, None) == -1
    for flag in (2, -1):
        p.bulk = flag
        assert lib.fdoct_angio_plan(C.byref(p), 6, 3, 20, C.byref(info)) == -1
    p.bulk, p.repeats = 1, 1 << 30
    assert lib.fdoct_angio_plan(C.byref(p), 6, 3, 20, C.byref(info)) == -1
    assert (info.groups, info.tiles, info.workgroups, info.workspace_bytes) == (-5, -6, -7, 8)
    # a range is not read without the correction
    q = angiography.params(repeats=3)
    q.bulk_first, q.bulk_count = 99, -4
    assert lib.fdoct_angio_plan(C.byref(q), 6, 3, 20, C.byref(info)) == 0 and info.workspace_bytes == 0


def test_params_behaves():
    p = angiography.params()
    assert (p.repeats, p.win_ascans, p.win_depths, p.bulk, p.bulk_first, p.bulk_count, p.min_power) == (2, 1, 1, 0, 0, 0, 0.0)
    p = angiography.params(repeats=4, win=(3, 5), bulk=True, min_power=2.5)
    assert (p.repeats, p.win_ascans, p.win_depths, p.bulk, p.bulk_first, p.bulk_count, p.min_power) == (4, 3, 5, 1, 0, 0, 2.5)
    p = angiography.params(repeats=8, bulk=(7, 9))
    assert (p.bulk, p.bulk_first, p.bulk_count) == (1, 7, 9)
    assert angiography.params(bulk=False).bulk == 0 and angiography.params(bulk=None).bulk == 0
    for bad in (dict(win=3), dict(win=(1, 2, 3)), dict(bulk=5), dict(bulk=(1, 2, 3)), dict(repeats="x"), dict(min_power="much"), dict(win=("a", 1))):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            angiography.params(**bad)
        assert e.value.code == -1, bad


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=128, numdisplaypoints=64)
    X = np.zeros((6, 3, 20), np.complex64)
    for bad in (X.astype(np.complex128), X.view(np.float32), np.zeros((6, 60), np.complex64), np.zeros((0, 3, 20), np.complex64)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            angiography.angio(rec, bad, GOOD)
        assert e.value.code == -1 and "complex64" in str(e.value)
    for kw in (dict(want=()), dict(want=("var", "phase")), dict(want=("var", "var")), dict(want="table")):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            angiography.angio(rec, X, GOOD, **kw)
        assert e.value.code == -1, kw
    for bad in (dict(repeats=4), dict(win=(17, 1)), dict(bulk=(20, 0)), dict(min_power=-1.0)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            angiography.angio(rec, X, dict(GOOD, **bad))
        assert e.value.code == -1, bad
    frames = np.zeros((3, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        angiography.process_angio(rec, frames.astype(np.int64), GOOD)
    assert e.value.code == -1 and "dtype" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        angiography.process_angio(rec, frames[:2], GOOD)       # two frames of three repeats
    assert e.value.code == -1
    for call in (lambda: angiography.angio(rec, X, GOOD, want="var"), lambda: angiography.process_angio(rec, frames, GOOD),
                 lambda: angiography.angio_device(rec, 4096, 6, 3, 20, GOOD, 8192, None, None, None),
                 lambda: angiography.process_angio_device(rec, 4096, capi.DTYPE_U16, 3, 16, GOOD, None, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = None
