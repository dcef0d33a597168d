"""CPU tests of the en-face stage's boundary (include/fdoct_enface.h): libfdoct_enface.so exports exactly the header's symbols and
the other libraries none of them, it needs libfdoct_hip.so and finds it through $ORIGIN, the entry points are function-try-blocks,
the header compiles as C99 next to fdoct.h, the ctypes mirrors have the structs' layout, a NULL handle is refused with the outputs
untouched, fdoct_enface_plan gives every refusal of the header's list that its arguments can show (the pointers', memory spaces'
and overlaps' need a call: tests/test_gpu_enface.py) with no GPU, its numbers are worked by hand at two shapes, and the binding
checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
from fdoct_amd import angiography, capi, coherent, dispersion, enface, ssada, vibrometry
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_enface_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_enface.h")
    assert declared == sorted(enface.ENFACE_ABI_SYMBOLS) == ["fdoct_enface", "fdoct_enface_plan", "fdoct_process_enface"]
    assert _exports(enface.library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path(), capi.doppler_library_path(),
                  dispersion.library_path(), vibrometry.library_path(), angiography.library_path(), coherent.library_path(), ssada.library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(enface.library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS +
              capi.DOPPLER_ABI_SYMBOLS + dispersion.DISPERSION_ABI_SYMBOLS + vibrometry.VIBRO_ABI_SYMBOLS + angiography.ANGIO_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    dyn = subprocess.check_output(["readelf", "-d", enface.library_path()], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", dyn)
    runpath = re.findall(r"\((?:RUNPATH|RPATH)\)\s+Library (?:runpath|rpath): \[([^\]]+)\]", dyn)
    assert "libfdoct_hip.so" in needed and not [n for n in needed if n.startswith("libfdoct_") and n != "libfdoct_hip.so"]
    assert runpath and "$ORIGIN" in runpath[0].split(":")
    # functions over a Reconstructor, not methods of it; the device-memory forms are *_into (the module's docstring says why)
    for name in ("library_path", "params", "plan", "project", "project_into", "process_project", "process_project_into", "attach"):
        assert callable(getattr(enface, name)) and not hasattr(capi.Reconstructor, name)
    assert not [n for n in dir(enface) if n.endswith("_device")]


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_enface.cpp"))
    assert [d[0] for d in defs] == enface.ENFACE_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_enface_header_compiles_as_c99_and_the_mirrors_have_its_layout(tmp_path):
    src = tmp_path / "use_enface.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "fdoct.h"
#include "fdoct_enface.h"
int main(void) {
  float v[2 * 3 * 5], out[4] = {7.f, 7.f, 7.f, 7.f};
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_enface_params p = {2, 1, 4, 2, 0.5, 3, 2, {0, -1}, {2, 3}};
  fdoct_enface_info info;
  int i;
  for (i = 0; i < 30; i++) v[i] = 1.f;
  if (fdoct_enface_plan(&p, 2, 3, 5, &info) != FDOCT_OK || info.ascans != 6 || info.workgroups != 2) return 1;
  if (info.workspace_bytes != 6 * 4 || info.read_first != 0 || info.read_count != 0) return 2;
  info.ascans = -3;
  p.median = 4;
  if (fdoct_enface_plan(&p, 2, 3, 5, &info) != FDOCT_ERR_INVALID || info.ascans != -3) return 3;
  p.median = 3;
  if (fdoct_enface(NULL, v, NULL, FDOCT_MEM_HOST, 2, 3, 5, &p, out, NULL, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 4;
  if (fdoct_process_enface(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 2, 0, FDOCT_ENFACE_SOURCE_DB, &p, out, NULL, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID)
    return 5;
  if (out[0] != 7.f || out[3] != 7.f) return 6;
  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d", (int)sizeof(fdoct_enface_params), (int)offsetof(fdoct_enface_params, smooth),
         (int)offsetof(fdoct_enface_params, threshold), (int)offsetof(fdoct_enface_params, median), (int)offsetof(fdoct_enface_params, slab_first),
         (int)offsetof(fdoct_enface_params, slab_count), (int)sizeof(fdoct_enface_info), (int)offsetof(fdoct_enface_info, workgroups),
         (int)offsetof(fdoct_enface_info, workspace_bytes), (int)offsetof(fdoct_enface_info, read_count), FDOCT_ENFACE_MAX_SLABS,
         FDOCT_ENFACE_MAX_SMOOTH, FDOCT_ENFACE_MAX_MEDIAN);
  return 0;
}
""")
    exe = tmp_path / "use_enface"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_enface", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    done = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.returncode
    P, I = enface._CParams, enface._CInfo
    assert [int(v) for v in done.stdout.split()] == [C.sizeof(P), P.smooth.offset, P.threshold.offset, P.median.offset, P.slab_first.offset,
                                                     P.slab_count.offset, C.sizeof(I), I.workgroups.offset, I.workspace_bytes.offset,
                                                     I.read_count.offset, enface.MAX_SLABS, enface.MAX_SMOOTH, enface.MAX_MEDIAN]
    assert C.sizeof(P) == 96 and C.sizeof(I) == 32


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    V = np.full(2 * 3 * 5, 2.0, np.float32)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(256, -7.0, np.float32) for _ in range(4)]
    p = enface.params(slabs=[(0, 2)], surface="absolute", threshold=1.0)
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_enface(None, V.ctypes.data, None, space, 2, 3, 5, p, *ptrs, space) == -1
        assert lib.fdoct_process_enface(None, frames.ctypes.data, capi.DTYPE_U16, space, 2, 0, 1, p, *ptrs, space) == -1
    assert lib.fdoct_enface(None, None, None, 0, 2, 3, 5, None, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(V == 2.0)


FIXED = dict(slabs=[(5, 10), (40, 100)])
SURF = dict(slabs=[(0, 64), (-10, 20)], surface="relative", threshold=0.5, smooth=4, median=5)
# (params' keywords, positions, H, D) -> (ascans, workgroups, workspace_bytes, read_first, read_count), or the refusal's code
PLAN_CASES = [
    # by hand: 2 x 3 A-scans, one wavefront each, four a workgroup: 2 workgroups; no surface: no workspace; the slabs clipped to 67
    # depths are [5, 15) and [40, 67): from depth 5, 62 depths
    ((FIXED, 2, 3, 67), (6, 2, 0, 5, 62)),
    # by hand: 256000 A-scans want 64000 workgroups, 256 compute units hold 8 each: 2048; one int32 raw surface each
    ((SURF, 256, 1000, 1024), (256000, 2048, 1024000, 0, 0)),
    ((dict(slabs=[(0, 1)]), 1, 1, 1), (1, 1, 0, 0, 1)), ((dict(slabs=[(3, 2), (1, 1)]), 65536, 1, 20), (65536, 2048, 0, 1, 4)),
    ((SURF, 1, 1 << 12, 1 << 12), (4096, 1024, 4096 * 4, 0, 0)),                                           # 2^24 pixels
    # positions outside 1..65536
    ((FIXED, 0, 3, 67), -1), ((FIXED, -1, 3, 67), -1), ((FIXED, 65537, 3, 67), -1),
    # ascans or depths below 1, or their product above 2^24
    ((FIXED, 2, 0, 67), -1), ((FIXED, 2, 3, 0), -1), ((FIXED, 2, -3, 67), -1), ((FIXED, 2, 3, -67), -1), ((FIXED, 2, 1 << 12, (1 << 12) + 1), -1),
    ((FIXED, 2, 1 << 16, 1 << 16), -1),
    # surface outside 0..2
    ((dict(SURF, surface=3), 2, 3, 67), -1), ((dict(SURF, surface=-1), 2, 3, 67), -1),
    # smooth outside 1..16
    ((dict(SURF, smooth=0), 2, 3, 67), -1), ((dict(SURF, smooth=17), 2, 3, 67), -1), ((dict(FIXED, smooth=0), 2, 3, 67), -1),
    ((dict(SURF, smooth=16), 2, 3, 67), (6, 2, 24, 0, 0)), ((dict(SURF, smooth=1), 2, 3, 67), (6, 2, 24, 0, 0)),
    # a search range outside [0, depths) or shorter than smooth
    ((dict(SURF, search=(67, 0)), 2, 3, 67), -1), ((dict(SURF, search=(-1, 0)), 2, 3, 67), -1), ((dict(SURF, search=(0, 68)), 2, 3, 67), -1),
    ((dict(SURF, search=(60, 8)), 2, 3, 67), -1), ((dict(SURF, search=(5, -1)), 2, 3, 67), -1), ((dict(SURF, search=(10, 3)), 2, 3, 67), -1),
    ((dict(SURF, search=(64, 0)), 2, 3, 67), -1), ((dict(SURF, search=(63, 0)), 2, 3, 67), (6, 2, 24, 0, 0)),
    ((dict(SURF, search=(10, 4)), 2, 3, 67), (6, 2, 24, 0, 0)), ((dict(SURF, search=(0, 67)), 2, 3, 67), (6, 2, 24, 0, 0)),
    # a threshold that is not finite, or in mode 2 is <= 0 or > 1
    ((dict(SURF, threshold=float("nan")), 2, 3, 67), -1), ((dict(SURF, threshold=float("inf")), 2, 3, 67), -1),
    ((dict(SURF, surface="absolute", threshold=float("-inf")), 2, 3, 67), -1), ((dict(SURF, threshold=0.0), 2, 3, 67), -1),
    ((dict(SURF, threshold=-0.5), 2, 3, 67), -1), ((dict(SURF, threshold=1.0000001), 2, 3, 67), -1), ((dict(SURF, threshold=1.0), 2, 3, 67), (6, 2, 24, 0, 0)),
    ((dict(SURF, surface="absolute", threshold=-70.0), 2, 3, 67), (6, 2, 24, 0, 0)), ((dict(SURF, surface="absolute", threshold=0.0), 2, 3, 67), (6, 2, 24, 0, 0)),
    # median even or outside 1..15
    ((dict(SURF, median=0), 2, 3, 67), -1), ((dict(SURF, median=4), 2, 3, 67), -1), ((dict(SURF, median=17), 2, 3, 67), -1), ((dict(SURF, median=-3), 2, 3, 67), -1),
    ((dict(FIXED, median=2), 2, 3, 67), -1), ((dict(SURF, median=15), 2, 3, 67), (6, 2, 24, 0, 0)), ((dict(SURF, median=1), 2, 3, 67), (6, 2, 24, 0, 0)),
    # nslabs outside 1..8
    ((dict(FIXED, slabs=[]), 2, 3, 67), -1), ((dict(FIXED, slabs=[(i, 1) for i in range(8)]), 2, 3, 67), (6, 2, 0, 0, 8)),
    # slab_count < 1
    ((dict(FIXED, slabs=[(5, 0)]), 2, 3, 67), -1), ((dict(FIXED, slabs=[(5, 10), (5, -2)]), 2, 3, 67), -1), ((dict(SURF, slabs=[(0, 0)]), 2, 3, 67), -1),
    ((dict(FIXED, slabs=[(5, (1 << 31) - 1)]), 2, 3, 67), (6, 2, 0, 5, 62)),
    # with surface = 0, a slab_first outside [0, depths)
    ((dict(FIXED, slabs=[(-1, 10)]), 2, 3, 67), -1), ((dict(FIXED, slabs=[(67, 1)]), 2, 3, 67), -1), ((dict(FIXED, slabs=[(66, 1)]), 2, 3, 67), (6, 2, 0, 66, 1)),
    # with a surface, |slab_first| >= depths
    ((dict(SURF, slabs=[(67, 1)]), 2, 3, 67), -1), ((dict(SURF, slabs=[(-67, 100)]), 2, 3, 67), -1), ((dict(SURF, slabs=[(-66, 100), (66, 1)]), 2, 3, 67), (6, 2, 24, 0, 0)),
]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[str(i) + " " + str(c[0][0])[:60] for i, c in enumerate(PLAN_CASES)])
def test_enface_plan(case):
    (kw, P, H, D), want = case
    if isinstance(want, int):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            enface.plan(kw, P, H, D)
        assert e.value.code == want
    else:
        p = enface.plan(kw, P, H, D)
        assert (p["ascans"], p["workgroups"], p["workspace_bytes"], p["read_first"], p["read_count"]) == want


def test_enface_plan_refuses_missing_pointers_and_a_ninth_slab_and_leaves_its_output_alone():
    lib = fdoct_amd.load_library()
    p, info = enface.params(**FIXED), enface._CInfo(-5, -6, 7, -8, -9)
    assert lib.fdoct_enface_plan(None, 2, 3, 67, C.byref(info)) == -1
    assert lib.fdoct_enface_plan(C.byref(p), 2, 3, 67, None) == -1
    for n in (9, 0, -1, 1 << 30):
        p.nslabs = n
        assert lib.fdoct_enface_plan(C.byref(p), 2, 3, 67, C.byref(info)) == -1
    assert (info.ascans, info.workgroups, info.workspace_bytes, info.read_first, info.read_count) == (-5, -6, 7, -8, -9)
    # without a surface neither the search range nor the threshold is read
    q = enface.params(**FIXED)
    q.search_first, q.search_count, q.threshold = 99, -4, float("nan")
    assert lib.fdoct_enface_plan(C.byref(q), 2, 3, 67, C.byref(info)) == 0 and info.workspace_bytes == 0


def test_params_behaves():
    p = enface.params()
    assert (p.surface, p.search_first, p.search_count, p.smooth, p.threshold, p.median, p.nslabs) == (0, 0, 0, 1, 0.0, 1, 1)
    assert (p.slab_first[0], p.slab_count[0]) == (0, 1)
    p = enface.params(slabs=[(3, 4), (-5, 6)], surface="relative", search=(7, 8), smooth=9, threshold=0.25, median=11)
    assert (p.surface, p.search_first, p.search_count, p.smooth, p.threshold, p.median, p.nslabs) == (2, 7, 8, 9, 0.25, 11, 2)
    assert (p.slab_first[1], p.slab_count[1]) == (-5, 6)
    assert enface.params(surface="absolute").surface == 1 and enface.params(surface=None).surface == 0
    for bad in (dict(slabs=3), dict(slabs=[(1, 2, 3)]), dict(slabs=[(0, 1)] * 9), dict(surface="steep"), dict(search=5), dict(smooth="x"),
                dict(threshold="much"), dict(slabs=[("a", 1)])):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            enface.params(**bad)
        assert e.value.code == -1, bad


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=128, numdisplaypoints=64)
    V = np.zeros((2, 3, 67), np.float32)
    for bad in (V.astype(np.float64), np.zeros((6, 67), np.float32), np.zeros((0, 3, 67), np.float32)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            enface.project(rec, bad, FIXED)
        assert e.value.code == -1 and "float32" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        enface.project(rec, V, SURF, structure=V[:1])
    assert e.value.code == -1 and "structure" in str(e.value)
    for kw in (dict(want=()), dict(want=("mean", "phase")), dict(want=("mean", "mean")), dict(want="table")):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            enface.project(rec, V, FIXED, **kw)
        assert e.value.code == -1, kw
    for bad in (dict(median=2), dict(smooth=17), dict(slabs=[(67, 1)])):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            enface.project(rec, V, dict(SURF, **bad))
        assert e.value.code == -1, bad
    frames = np.zeros((3, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        enface.process_project(rec, frames.astype(np.int64), FIXED)
    assert e.value.code == -1 and "dtype" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        enface.process_project(rec, frames, FIXED, source="phase")
    assert e.value.code == -1 and "source" in str(e.value)
    for call in (lambda: enface.project(rec, V, FIXED, want="mean"), lambda: enface.process_project(rec, frames, dict(slabs=[(5, 10)])),
                 lambda: enface.project_into(rec, 4096, None, 2, 3, 67, FIXED, 8192, None, None, None),
                 lambda: enface.process_project_into(rec, 4096, capi.DTYPE_U16, 3, 16, "db", dict(slabs=[(5, 10)]), None, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = None
