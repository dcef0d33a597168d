"""CPU tests of the split-spectrum stage's boundary (include/fdoct_ssada.h): libfdoct_ssada.so exports exactly the header's symbols
and the other eight libraries none of them, it needs libfdoct_hip.so and finds it through $ORIGIN, the core library's exported
symbols are still the closed set of its headers, the entry points are function-try-blocks, the header compiles as C99 next to
fdoct.h, the ctypes mirrors have the structs' layout, a NULL handle is refused with the outputs untouched, fdoct_ssada_plan gives
every refusal of the header's list that its arguments can show (the pointers', memory spaces' and overlaps' need a call:
tests/test_gpu_ssada.py) and the pass rule with no GPU, and the binding checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
import ssada_cases as sc
from fdoct_amd import angiography, capi, coherent, dispersion, ssada, vibrometry
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_ssada_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_ssada.h")
    assert declared == sorted(ssada.SSADA_ABI_SYMBOLS) == ["fdoct_process_ssada", "fdoct_ssada", "fdoct_ssada_band_table", "fdoct_ssada_plan"]
    assert _exports(ssada.library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path(), capi.doppler_library_path(),
                  dispersion.library_path(), vibrometry.library_path(), angiography.library_path(), coherent.library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(ssada.library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS +
              capi.DOPPLER_ABI_SYMBOLS + dispersion.DISPERSION_ABI_SYMBOLS + vibrometry.VIBRO_ABI_SYMBOLS + angiography.ANGIO_ABI_SYMBOLS +
              coherent.CXAVG_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    needed = subprocess.check_output(["readelf", "-d", ssada.library_path()], text=True)
    assert "libfdoct_hip.so" in needed and "$ORIGIN" in needed and "libfdoct_angio" not in needed    # the window stage is linked in
    # functions over a Reconstructor, not methods of it
    for name in ("library_path", "params", "plan", "band_table", "ssada", "ssada_device", "process_ssada", "process_ssada_device", "attach"):
        assert callable(getattr(ssada, name)) and not hasattr(capi.Reconstructor, name)


def test_the_core_librarys_symbols_are_still_the_closed_set_of_its_headers():
    core = set(capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
               capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS)
    assert _exports(fdoct_amd.library_path()) == core


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_ssada.cpp"))
    assert [d[0] for d in defs] == ssada.SSADA_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_ssada_header_compiles_as_c99_and_the_mirrors_have_its_layout(tmp_path):
    src = tmp_path / "use_ssada.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "fdoct.h"
#include "fdoct_ssada.h"
int main(void) {
  float x[2 * 4 * 3 * 16], out[4] = {7.f, 7.f, 7.f, 7.f}, table[2 * 16];
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_ssada_params p = {2, 2, 4.0, 0, 0, 0, 0, 3, 5, 0.0, 0};
  fdoct_ssada_info info;
  int i;
  for (i = 0; i < 384; i++) x[i] = 1.f;
  if (fdoct_ssada_plan(&p, 4, 3, 16, &info) != FDOCT_OK || info.groups != 2 || info.depth_count != 8 || info.groups_per_pass != 2 || info.passes != 1) return 1;
  if (info.lds_bytes != 3 * 16 * 8 || info.workgroups != 12 || info.workspace_bytes != 2 * 2 * 3 * 8 * (8 * 2 + 8)) return 2;
  info.groups = -3;
  p.repeats = 3;
  if (fdoct_ssada_plan(&p, 4, 3, 16, &info) != FDOCT_ERR_INVALID || info.groups != -3) return 3;
  p.repeats = 2;
  if (fdoct_ssada_plan(&p, 4, 3, 17, &info) != FDOCT_ERR_UNSUPPORTED || info.groups != -3) return 4;
  if (fdoct_ssada_band_table(&p, 16, table) != FDOCT_OK || table[0] <= 0.f || table[31] <= 0.f) return 5;
  if (fdoct_ssada(NULL, x, FDOCT_MEM_HOST, 4, 3, 16, &p, out, NULL, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 6;
  if (fdoct_process_ssada(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 2, 0, &p, out, NULL, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 7;
  if (out[0] != 7.f || out[3] != 7.f) return 8;
  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", (int)sizeof(fdoct_ssada_params), (int)offsetof(fdoct_ssada_params, sigma),
         (int)offsetof(fdoct_ssada_params, k_first), (int)offsetof(fdoct_ssada_params, depth_count), (int)offsetof(fdoct_ssada_params, win_depths),
         (int)offsetof(fdoct_ssada_params, min_power), (int)offsetof(fdoct_ssada_params, max_workspace_bytes), (int)sizeof(fdoct_ssada_info),
         (int)offsetof(fdoct_ssada_info, passes), (int)offsetof(fdoct_ssada_info, lds_bytes), (int)offsetof(fdoct_ssada_info, workgroups),
         (int)offsetof(fdoct_ssada_info, workspace_bytes), FDOCT_SSADA_MAX_WIN, FDOCT_SSADA_MAX_REPEATS, FDOCT_SSADA_MAX_BANDS);
  return 0;
}
""")
    exe = tmp_path / "use_ssada"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_ssada", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    done = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.returncode
    P, I = ssada._CParams, ssada._CInfo
    assert [int(v) for v in done.stdout.split()] == [C.sizeof(P), P.sigma.offset, P.k_first.offset, P.depth_count.offset, P.win_depths.offset,
                                                     P.min_power.offset, P.max_workspace_bytes.offset, C.sizeof(I), I.passes.offset, I.lds_bytes.offset,
                                                     I.workgroups.offset, I.workspace_bytes.offset, ssada.MAX_WIN, ssada.MAX_REPEATS, ssada.MAX_BANDS]
    assert C.sizeof(P) == 56 and C.sizeof(I) == 40


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    X = np.full(4 * 3 * 16, 2 + 1j, np.complex64)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(4096, -7.0, np.float32) for _ in range(4)]
    p = ssada.params(repeats=2, bands=2, n=16)
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_ssada(None, X.ctypes.data, space, 4, 3, 16, p, *ptrs, space) == -1
        assert lib.fdoct_process_ssada(None, frames.ctypes.data, capi.DTYPE_U16, space, 2, 0, p, *ptrs, space) == -1
    assert lib.fdoct_ssada(None, None, 0, 4, 3, 16, None, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(X == np.complex64(2 + 1j))


GOOD = dict(repeats=3, bands=4, sigma=5.0, support=(4, 40), depth=(2, 20), win=(3, 5))
SHARE = 4 * 3 * 20 * (8 * 3 + 8)     # a group of GOOD at 3 A-scans: bands x ascans x depths x (8 R + 8)
# (params' keywords, nframes, ascans, n) -> the refusal's code, or None where the call is accepted
REFUSALS = [
    ((GOOD, 6, 3, 60), None),
    # n: a prime factor above 5, or outside 16 .. 4096: unsupported; below 1: invalid
    ((GOOD, 6, 3, 56), -2), ((GOOD, 6, 3, 4097), -2), ((GOOD, 6, 3, 8192), -2), ((dict(GOOD, support=(0, 0), depth=(0, 0)), 6, 3, 15), -2),
    ((dict(GOOD, support=(0, 0), depth=(0, 0)), 6, 3, 8), -2), ((GOOD, 6, 3, 0), -1), ((GOOD, 6, 3, -60), -1),
    ((dict(GOOD, support=(0, 0), depth=(0, 0)), 6, 3, 16), None), ((GOOD, 6, 3, 4096), None), ((GOOD, 6, 3, 3000), None),
    # repeats outside 2 .. 64, bands outside 1 .. 16
    ((dict(GOOD, repeats=1), 6, 3, 60), -1), ((dict(GOOD, repeats=0), 6, 3, 60), -1), ((dict(GOOD, repeats=65), 130, 3, 60), -1),
    ((dict(GOOD, repeats=64), 64, 3, 60), None), ((dict(GOOD, bands=0), 6, 3, 60), -1), ((dict(GOOD, bands=17), 6, 3, 60), -1),
    ((dict(GOOD, bands=-4), 6, 3, 60), -1), ((dict(GOOD, bands=16), 6, 3, 60), None), ((dict(GOOD, bands=1), 6, 3, 60), None),
    # nframes not a positive multiple of repeats, or nframes x bands above 65536
    ((GOOD, 7, 3, 60), -1), ((GOOD, 2, 3, 60), -1), ((GOOD, 0, 3, 60), -1), ((GOOD, -3, 3, 60), -1),
    ((dict(GOOD, repeats=2, depth=(2, 1)), 16384, 1, 60), None), ((dict(GOOD, repeats=2, depth=(2, 1)), 16386, 1, 60), -1),
    ((dict(GOOD, repeats=2, bands=1, depth=(2, 1)), 65536, 1, 60), None), ((dict(GOOD, repeats=2, bands=1, depth=(2, 1)), 65538, 1, 60), -1),
    # ascans below 1, or ascans x depths kept above 2^24
    ((GOOD, 6, 0, 60), -1), ((GOOD, 6, -3, 60), -1), ((dict(GOOD, bands=1, depth=(0, 16)), 6, 1 << 20, 60), None),
    ((dict(GOOD, bands=1, depth=(0, 17)), 6, 1 << 20, 60), -1),
    # the support: inside [0, n), with a bin
    ((dict(GOOD, support=(0, 0)), 6, 3, 60), None), ((dict(GOOD, support=(59, 1)), 6, 3, 60), None), ((dict(GOOD, support=(59, 0)), 6, 3, 60), None),
    ((dict(GOOD, support=(20, 3)), 6, 3, 60), None), ((dict(GOOD, support=(60, 0)), 6, 3, 60), -1), ((dict(GOOD, support=(-1, 0)), 6, 3, 60), -1),
    ((dict(GOOD, support=(0, 61)), 6, 3, 60), -1), ((dict(GOOD, support=(59, 2)), 6, 3, 60), -1), ((dict(GOOD, support=(5, -1)), 6, 3, 60), -1),
    # the depth range: inside [0, n), with a bin (count 0: up to n / 2)
    ((dict(GOOD, depth=(0, 0)), 6, 3, 60), None), ((dict(GOOD, depth=(29, 0)), 6, 3, 60), None), ((dict(GOOD, depth=(30, 0)), 6, 3, 60), -1),
    ((dict(GOOD, depth=(45, 0)), 6, 3, 60), -1), ((dict(GOOD, depth=(0, 60)), 6, 3, 60), None), ((dict(GOOD, depth=(59, 1)), 6, 3, 60), None),
    ((dict(GOOD, depth=(0, 61)), 6, 3, 60), -1), ((dict(GOOD, depth=(60, 0)), 6, 3, 60), -1), ((dict(GOOD, depth=(-1, 4)), 6, 3, 60), -1),
    ((dict(GOOD, depth=(58, 3)), 6, 3, 60), -1), ((dict(GOOD, depth=(5, -1)), 6, 3, 60), -1),
    # sigma finite and > 0
    ((dict(GOOD, sigma=0.0), 6, 3, 60), -1), ((dict(GOOD, sigma=-1.0), 6, 3, 60), -1), ((dict(GOOD, sigma=float("nan")), 6, 3, 60), -1),
    ((dict(GOOD, sigma=float("inf")), 6, 3, 60), -1), ((dict(GOOD, sigma=1e12), 6, 3, 60), None), ((dict(GOOD, sigma=1e-3), 6, 3, 60), None),
    # a window size outside 1 .. 16
    ((dict(GOOD, win=(0, 5)), 6, 3, 60), -1), ((dict(GOOD, win=(3, 0)), 6, 3, 60), -1), ((dict(GOOD, win=(17, 5)), 6, 3, 60), -1),
    ((dict(GOOD, win=(3, 17)), 6, 3, 60), -1), ((dict(GOOD, win=(16, 16)), 6, 3, 60), None), ((dict(GOOD, win=(1, 1)), 6, 3, 60), None),
    # min_power not finite or negative
    ((dict(GOOD, min_power=float("nan")), 6, 3, 60), -1), ((dict(GOOD, min_power=float("inf")), 6, 3, 60), -1), ((dict(GOOD, min_power=-1e-30), 6, 3, 60), -1),
    ((dict(GOOD, min_power=2.5), 6, 3, 60), None),
    # a cap below one group
    ((dict(GOOD, max_workspace_bytes=SHARE - 1), 6, 3, 60), -1), ((dict(GOOD, max_workspace_bytes=SHARE), 6, 3, 60), None),
    ((dict(GOOD, max_workspace_bytes=1), 6, 3, 60), -1),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[str(c[0]) for c in REFUSALS])
def test_ssada_plan_refusals_one_by_one(case):
    (kw, T, H, n), want = case
    if want is None:
        p = ssada.plan(kw, T, H, n)
        assert p == sc.plan(T, kw["repeats"], kw["bands"], H, n, kw["depth"], kw.get("max_workspace_bytes", 0))
    else:
        with pytest.raises(fdoct_amd.FdoctError) as e:
            ssada.plan(kw, T, H, n)
        assert e.value.code == want


def test_the_pass_rule():
    kw = dict(GOOD)
    T, H, n = 7 * 3, 3, 60                                    # seven groups
    one = ssada.plan(kw, T, H, n)                            # cap 0: 2 GiB, one pass
    assert (one["groups"], one["groups_per_pass"], one["passes"], one["workspace_bytes"]) == (7, 7, 1, 7 * SHARE)
    three = ssada.plan(dict(kw, max_workspace_bytes=3 * SHARE + SHARE // 2), T, H, n)      # three groups and a half fit: 3 + 3 + 1
    assert (three["groups_per_pass"], three["passes"], three["workspace_bytes"]) == (3, 3, 3 * SHARE)
    assert three["workgroups"] == 3 * 3 * 3 and one["workgroups"] == 7 * 3 * 3
    single = ssada.plan(dict(kw, max_workspace_bytes=SHARE), T, H, n)
    assert (single["groups_per_pass"], single["passes"], single["workspace_bytes"]) == (1, 7, SHARE)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        ssada.plan(dict(kw, max_workspace_bytes=SHARE - 1), T, H, n)
    assert e.value.code == -1
    # the default cap is 2 GiB: 64 frames of 1000 x 1024 kept in four bands are 2 GB of pairs and 0.26 GB of d and p -- two passes
    big = ssada.plan(dict(repeats=4, bands=4, sigma=100.0), 64, 1000, 2048)
    share = sc.group_share(4, 4, 1000, 1024)
    assert big["groups_per_pass"] == (2 << 30) // share and big["passes"] == -(-16 // big["groups_per_pass"]) and big["workspace_bytes"] <= 2 << 30
    assert big["lds_bytes"] == 3 * 2048 * 8 and big["workgroups"] == 2048


def test_ssada_plan_refuses_missing_pointers_and_leaves_its_output_alone():
    lib = fdoct_amd.load_library()
    p, info = ssada.params(**GOOD), ssada._CInfo(-5, -6, -7, -8, 9, -10, 11)
    assert lib.fdoct_ssada_plan(None, 6, 3, 60, C.byref(info)) == -1
    assert lib.fdoct_ssada_plan(C.byref(p), 6, 3, 60, None) == -1
    p.repeats = 1 << 30
    assert lib.fdoct_ssada_plan(C.byref(p), 6, 3, 60, C.byref(info)) == -1
    assert (info.groups, info.depth_count, info.groups_per_pass, info.passes, info.lds_bytes, info.workgroups, info.workspace_bytes) == (-5, -6, -7, -8, 9, -10, 11)
    table = np.full(4 * 60 + 1, -7.0, np.float32)
    q = ssada.params(**GOOD)
    assert lib.fdoct_ssada_band_table(None, 60, table.ctypes.data) == -1 and lib.fdoct_ssada_band_table(C.byref(q), 60, None) == -1
    assert lib.fdoct_ssada_band_table(C.byref(q), 0, table.ctypes.data) == -1 and lib.fdoct_ssada_band_table(C.byref(q), 43, table.ctypes.data) == -1
    for bad in (dict(bands=0), dict(bands=17), dict(sigma=0.0), dict(sigma=float("nan")), dict(support=(60, 0)), dict(support=(0, 61))):
        b = ssada.params(**dict(GOOD, **bad))
        assert lib.fdoct_ssada_band_table(C.byref(b), 60, table.ctypes.data) == -1, bad
    assert np.all(table == -7.0)
    assert lib.fdoct_ssada_band_table(C.byref(q), 60, table.ctypes.data) == 0 and table[-1] == -7.0 and np.all(table[:-1] >= 0)
    # the table needs no transform: a length the stage refuses is fine
    assert ssada.band_table(dict(repeats=2, bands=3, sigma=2.0), 7).shape == (3, 7)


def test_params_behaves():
    p = ssada.params(n=2048)
    assert (p.repeats, p.bands, p.sigma, p.k_first, p.k_count, p.depth_first, p.depth_count, p.win_ascans, p.win_depths, p.min_power,
            p.max_workspace_bytes) == (2, 4, 256.0, 0, 0, 0, 0, 1, 1, 0.0, 0)
    assert ssada.params(bands=4, support=(100, 800)).sigma == 100.0 and ssada.params(bands=2, support=(100, 0), n=1100).sigma == 250.0
    p = ssada.params(repeats=4, bands=3, sigma=7.5, support=(1, 2), depth=(3, 4), win=(5, 6), min_power=2.5, max_workspace_bytes=1 << 33)
    assert (p.repeats, p.bands, p.sigma, p.k_first, p.k_count, p.depth_first, p.depth_count, p.win_ascans, p.win_depths, p.min_power,
            p.max_workspace_bytes) == (4, 3, 7.5, 1, 2, 3, 4, 5, 6, 2.5, 1 << 33)
    for bad in (dict(win=3), dict(win=(1, 2, 3)), dict(support=5), dict(depth=(1, 2, 3)), dict(repeats="x", sigma=1.0), dict(min_power="much", sigma=1.0),
                dict(sigma=None), dict(sigma=None, bands=0, n=16)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            ssada.params(**bad)
        assert e.value.code == -1, bad


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=3, numfftpoints=60, numdisplaypoints=60)
    X = np.zeros((6, 3, 60), np.complex64)
    for bad in (X.astype(np.complex128), X.view(np.float32), np.zeros((6, 180), np.complex64), np.zeros((0, 3, 60), np.complex64)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            ssada.ssada(rec, bad, GOOD)
        assert e.value.code == -1 and "complex64" in str(e.value)
    for kw in (dict(want=()), dict(want=("decorr", "phase")), dict(want=("bands", "bands")), dict(want="table")):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            ssada.ssada(rec, X, GOOD, **kw)
        assert e.value.code == -1, kw
    for bad in (dict(repeats=4), dict(win=(17, 1)), dict(depth=(60, 0)), dict(min_power=-1.0), dict(bands=17)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            ssada.ssada(rec, X, dict(GOOD, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(fdoct_amd.FdoctError) as e:
        ssada.ssada(rec, np.zeros((6, 3, 56), np.complex64), dict(GOOD, support=(0, 0), depth=(0, 0)))
    assert e.value.code == -2
    frames = np.zeros((3, 3, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        ssada.process_ssada(rec, frames.astype(np.int64), GOOD)
    assert e.value.code == -1 and "dtype" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        ssada.process_ssada(rec, frames[:2], GOOD)       # two frames of three repeats
    assert e.value.code == -1
    short = capi.Reconstructor.__new__(capi.Reconstructor)
    short.lib, short.h, short.cfg = rec.lib, None, fdoct_amd.Config(width=8, height=3, numfftpoints=120, numdisplaypoints=60)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        ssada.process_ssada(short, frames, GOOD)
    assert e.value.code == -2 and "numfftpoints" in str(e.value)
    short.h = None
    for call in (lambda: ssada.ssada(rec, X, GOOD, want="decorr"), lambda: ssada.process_ssada(rec, frames, GOOD),
                 lambda: ssada.ssada_device(rec, 4096, 6, 3, 60, GOOD, 8192, None, None, None),
                 lambda: ssada.process_ssada_device(rec, 4096, capi.DTYPE_U16, 3, 16, GOOD, None, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = None
