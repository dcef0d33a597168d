"""CPU tests of the coherent-averaging stage's boundary (include/fdoct_cxavg.h): libfdoct_cxavg.so exports exactly the header's
symbols and the other seven libraries none of them, it needs libfdoct_hip.so and finds it through $ORIGIN, the entry points are
function-try-blocks, the header compiles as C99 next to fdoct.h, the ctypes mirrors have the structs' layout, a NULL handle is
refused with the outputs untouched, fdoct_cxavg_plan gives every refusal of the header's list that its arguments can show (the
pointers', memory spaces' and overlaps' need a call: tests/test_gpu_cxavg.py) and the form and workspace of the restated launch
arithmetic with no GPU, and the binding checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cxavg_model as cm
import fdoct_amd
from fdoct_amd import angiography, capi, coherent, dispersion, vibrometry
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_cxavg_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_cxavg.h")
    assert declared == sorted(coherent.CXAVG_ABI_SYMBOLS) == ["fdoct_cxavg", "fdoct_cxavg_plan", "fdoct_process_cxavg"]
    assert _exports(coherent.library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path(), capi.doppler_library_path(),
                  dispersion.library_path(), vibrometry.library_path(), angiography.library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(coherent.library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS +
              capi.DOPPLER_ABI_SYMBOLS + dispersion.DISPERSION_ABI_SYMBOLS + vibrometry.VIBRO_ABI_SYMBOLS + angiography.ANGIO_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    needed = subprocess.check_output(["readelf", "-d", coherent.library_path()], text=True)
    assert "libfdoct_hip.so" in needed and "$ORIGIN" in needed
    # functions over a Reconstructor, not methods of it
    for name in ("library_path", "params", "plan", "cxavg", "cxavg_device", "process_cxavg", "process_cxavg_device", "attach"):
        assert callable(getattr(coherent, name)) and not hasattr(capi.Reconstructor, name)


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_cxavg.cpp"))
    assert [d[0] for d in defs] == coherent.CXAVG_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_cxavg_header_compiles_as_c99_and_the_mirrors_have_its_layout(tmp_path):
    src = tmp_path / "use_cxavg.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "fdoct.h"
#include "fdoct_cxavg.h"
int main(void) {
  float x[2 * 6 * 3 * 5], out[4] = {7.f, 7.f, 7.f, 7.f};
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_cxavg_params p = {3, 3, 1, 2, 1, 2};
  fdoct_cxavg_info info;
  int i;
  for (i = 0; i < 180; i++) x[i] = 1.f;
  if (fdoct_cxavg_plan(&p, 6, 3, 5, &info) != FDOCT_OK || info.groups != 2 || info.form != FDOCT_CXAVG_FORM_REGISTER || info.workgroups != 6) return 1;
  if (info.workspace_bytes != (2 * 3 + 2 * 3 * 3) * 8) return 2;
  info.groups = -3;
  p.repeats = 4;
  if (fdoct_cxavg_plan(&p, 6, 3, 5, &info) != FDOCT_ERR_INVALID || info.groups != -3) return 3;
  p.repeats = 3;
  if (fdoct_cxavg(NULL, x, FDOCT_MEM_HOST, 6, 3, 5, &p, NULL, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 4;
  if (fdoct_process_cxavg(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 2, 0, &p, NULL, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 5;
  if (out[0] != 7.f || out[3] != 7.f) return 6;
  printf("%d %d %d %d %d %d %d %d %d %d %d", (int)sizeof(fdoct_cxavg_params), (int)offsetof(fdoct_cxavg_params, stride),
         (int)offsetof(fdoct_cxavg_params, align), (int)offsetof(fdoct_cxavg_params, align_count), (int)sizeof(fdoct_cxavg_info),
         (int)offsetof(fdoct_cxavg_info, form), (int)offsetof(fdoct_cxavg_info, workgroups), (int)offsetof(fdoct_cxavg_info, workspace_bytes),
         FDOCT_CXAVG_MAX_REPEATS, FDOCT_CXAVG_REG_PAIRS, FDOCT_CXAVG_FORM_STREAMING);
  return 0;
}
""")
    exe = tmp_path / "use_cxavg"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_cxavg", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    done = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.returncode
    P, I = coherent._CParams, coherent._CInfo
    assert [int(v) for v in done.stdout.split()] == [C.sizeof(P), P.stride.offset, P.align.offset, P.align_count.offset, C.sizeof(I), I.form.offset,
                                                     I.workgroups.offset, I.workspace_bytes.offset, coherent.MAX_REPEATS, coherent.REG_PAIRS,
                                                     coherent.FORM_STREAMING]
    assert C.sizeof(P) == 24 and C.sizeof(I) == 24
    assert (coherent.REG_PAIRS, coherent.FORM_REGISTER, coherent.FORM_STREAMING) == (cm.REG_PAIRS, cm.FORM_REGISTER, cm.FORM_STREAMING)


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    X = np.full(4 * 3 * 5, 2 + 1j, np.complex64)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(256, -7.0, np.float32) for _ in range(4)]
    p = coherent.params(repeats=2, align=2)
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_cxavg(None, X.ctypes.data, space, 4, 3, 5, p, *ptrs, space) == -1
        assert lib.fdoct_process_cxavg(None, frames.ctypes.data, capi.DTYPE_U16, space, 2, 0, p, *ptrs, space) == -1
    assert lib.fdoct_cxavg(None, None, 0, 4, 3, 5, None, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(X == np.complex64(2 + 1j))


GOOD = dict(repeats=3, ref=1, align=1, align_range=(2, 3))
K, S = cm.FORM_REGISTER, cm.FORM_STREAMING
# (params' keywords, nframes, H, D) -> (groups, form, workgroups, workspace_bytes), or the refusal's code
PLAN_CASES = [
    ((GOOD, 6, 3, 20), (2, K, 6, 0)), ((GOOD, 3, 17, 65), (1, K, 17, 0)), ((dict(GOOD, align=2), 3, 17, 65), (1, K, 17, (3 + 3 * 17) * 8)),
    ((dict(GOOD, align=0), 3, 17, 65), (1, K, 17, 0)),
    ((dict(GOOD, repeats=2), 65536, 1, 20), (32768, K, 1024, 0)), ((dict(GOOD, repeats=64, align=2), 64, 3, 20), (1, S, 3, (64 + 64 * 3) * 8)),
    ((dict(GOOD, repeats=2, align=2), 2, 1 << 12, 1 << 12), (1, S, 1024, (2 + 2 * 4096) * 8)),                  # 2^24 pixels
    # the form: the repeats, rounded up to 2, 4, 8 or 16, times ceil(depths / 256) against 16 pairs a thread, whatever the rest
    ((dict(GOOD, repeats=4), 64, 1000, 1024), (16, K, 1024, 0)), ((dict(GOOD, repeats=4), 64, 1000, 1025), (16, S, 1024, 0)),
    ((dict(GOOD, repeats=2), 2, 1, 2048), (1, K, 1, 0)), ((dict(GOOD, repeats=2), 2, 1, 2049), (1, S, 1, 0)),
    ((dict(GOOD, repeats=16, ref=15), 16, 2, 256), (1, K, 2, 0)), ((dict(GOOD, repeats=16, ref=15), 16, 2, 257), (1, S, 2, 0)),
    ((dict(GOOD, repeats=9), 9, 2, 256), (1, K, 2, 0)), ((dict(GOOD, repeats=5), 5, 2, 512), (1, K, 2, 0)), ((dict(GOOD, repeats=5), 5, 2, 513), (1, S, 2, 0)),
    ((dict(GOOD, repeats=17), 17, 2, 20), (1, S, 2, 0)), ((dict(GOOD, repeats=64, ref=63), 64, 2, 20), (1, S, 2, 0)), ((GOOD, 3, 2, 1024), (1, K, 2, 0)),
    ((GOOD, 3, 2, 1025), (1, S, 2, 0)),
    # stride: the groups of a sliding call
    ((dict(GOOD, stride=1), 6, 3, 20), (4, K, 12, 0)), ((dict(GOOD, stride=1, align=2), 6, 3, 20), (4, K, 12, (12 + 12 * 3) * 8)),
    ((dict(GOOD, stride=2), 7, 3, 20), (3, K, 9, 0)), ((dict(GOOD, stride=3), 3, 3, 20), (1, K, 3, 0)),
    ((dict(GOOD, stride=0), 6, 3, 20), -1), ((dict(GOOD, stride=-1), 6, 3, 20), -1), ((dict(GOOD, stride=4), 7, 3, 20), -1),
    ((dict(GOOD, stride=2), 6, 3, 20), -1),                                                                      # (6 - 3) % 2
    # repeats outside 2..64
    ((dict(GOOD, repeats=1, ref=0), 6, 3, 20), -1), ((dict(GOOD, repeats=0, ref=0), 6, 3, 20), -1), ((dict(GOOD, repeats=-2), 6, 3, 20), -1),
    ((dict(GOOD, repeats=65), 130, 3, 20), -1),
    # nframes below repeats, off the stride, or above 65536
    ((GOOD, 7, 3, 20), -1), ((GOOD, 2, 3, 20), -1), ((GOOD, 0, 3, 20), -1), ((GOOD, -3, 3, 20), -1), ((GOOD, 65538, 3, 20), -1),
    ((dict(GOOD, repeats=2), 65538, 3, 20), -1), ((dict(GOOD, stride=1), 65537, 3, 20), -1), ((dict(GOOD, stride=1), 65536, 1, 20), (65534, K, 1024, 0)),
    # ref outside [0, repeats)
    ((dict(GOOD, ref=0), 6, 3, 20), (2, K, 6, 0)), ((dict(GOOD, ref=2), 6, 3, 20), (2, K, 6, 0)), ((dict(GOOD, ref=3), 6, 3, 20), -1),
    ((dict(GOOD, ref=-1), 6, 3, 20), -1),
    # align outside 0..2
    ((dict(GOOD, align=3), 6, 3, 20), -1), ((dict(GOOD, align=-1), 6, 3, 20), -1),
    # ascans or depths below 1, or their product above 2^24
    ((GOOD, 6, 0, 20), -1), ((GOOD, 6, 3, 0), -1), ((GOOD, 6, -3, 20), -1), ((GOOD, 6, 3, -20), -1), ((GOOD, 6, 1 << 12, (1 << 12) + 1), -1),
    ((GOOD, 6, 1 << 24, 5), -1), ((GOOD, 6, 1 << 16, 1 << 16), -1),
    # an alignment range outside [0, depths)
    ((dict(GOOD, align_range=(0, 0)), 6, 3, 20), (2, K, 6, 0)), ((dict(GOOD, align_range=(19, 1)), 6, 3, 20), (2, K, 6, 0)),
    ((dict(GOOD, align_range=(0, 20)), 6, 3, 20), (2, K, 6, 0)), ((dict(GOOD, align_range=(20, 0)), 6, 3, 20), -1),
    ((dict(GOOD, align_range=(-1, 0)), 6, 3, 20), -1), ((dict(GOOD, align_range=(0, 21)), 6, 3, 20), -1), ((dict(GOOD, align_range=(19, 2)), 6, 3, 20), -1),
    ((dict(GOOD, align_range=(5, -1)), 6, 3, 20), -1), ((dict(GOOD, align=2, align_range=(19, 2)), 6, 3, 20), -1),
]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[str(c[0]) for c in PLAN_CASES])
def test_cxavg_plan(case):
    (kw, T, H, D), want = case
    if isinstance(want, int):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            coherent.plan(kw, T, H, D)
        assert e.value.code == want
    else:
        p = coherent.plan(kw, T, H, D)
        assert (p["groups"], p["form"], p["workgroups"], p["workspace_bytes"]) == want
        assert want == cm.geometry(T, kw["repeats"], kw.get("stride"), H, D, kw["align"])       # the launch arithmetic restated


def test_cxavg_plan_refuses_missing_pointers_and_leaves_its_output_alone():
    lib = fdoct_amd.load_library()
    p, info = coherent.params(**GOOD), coherent._CInfo(-5, -6, -7, 8)
    assert lib.fdoct_cxavg_plan(None, 6, 3, 20, C.byref(info)) == -1
    assert lib.fdoct_cxavg_plan(C.byref(p), 6, 3, 20, None) == -1
    for bad in (dict(align=3), dict(repeats=1 << 30), dict(stride=0), dict(ref=3)):
        q = coherent.params(**GOOD)
        for k, v in bad.items():
            setattr(q, k, v)
        assert lib.fdoct_cxavg_plan(C.byref(q), 6, 3, 20, C.byref(info)) == -1, bad
    assert (info.groups, info.form, info.workgroups, info.workspace_bytes) == (-5, -6, -7, 8)
    # a range is not read without the alignment
    q = coherent.params(repeats=3, align=0)
    q.align_first, q.align_count = 99, -4
    assert lib.fdoct_cxavg_plan(C.byref(q), 6, 3, 20, C.byref(info)) == 0 and info.workspace_bytes == 0 and info.groups == 2


def test_params_behaves():
    p = coherent.params()
    assert (p.repeats, p.stride, p.ref, p.align, p.align_first, p.align_count) == (2, 2, 0, 1, 0, 0)
    p = coherent.params(repeats=4, stride=1, ref=3, align=2, align_range=(7, 9))
    assert (p.repeats, p.stride, p.ref, p.align, p.align_first, p.align_count) == (4, 1, 3, 2, 7, 9)
    assert coherent.params(repeats=8).stride == 8 and coherent.params(repeats=8, stride=None).stride == 8
    for bad in (dict(align_range=3), dict(align_range=(1, 2, 3)), dict(repeats="x"), dict(stride="s"), dict(ref=None), dict(align="row"),
                dict(align_range=("a", 1))):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            coherent.params(**bad)
        assert e.value.code == -1, bad


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=128, numdisplaypoints=64)
    X = np.zeros((6, 3, 20), np.complex64)
    for bad in (X.astype(np.complex128), X.view(np.float32), np.zeros((6, 60), np.complex64), np.zeros((0, 3, 20), np.complex64)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            coherent.cxavg(rec, bad, GOOD)
        assert e.value.code == -1 and "complex64" in str(e.value)
    for kw in (dict(want=()), dict(want=("mag", "phase")), dict(want=("mag", "mag")), dict(want="table")):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            coherent.cxavg(rec, X, GOOD, **kw)
        assert e.value.code == -1, kw
    for bad in (dict(repeats=4), dict(stride=2), dict(ref=3), dict(align=3), dict(align_range=(20, 0))):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            coherent.cxavg(rec, X, dict(GOOD, **bad))
        assert e.value.code == -1, bad
    frames = np.zeros((3, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        coherent.process_cxavg(rec, frames.astype(np.int64), GOOD)
    assert e.value.code == -1 and "dtype" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        coherent.process_cxavg(rec, frames[:2], GOOD)       # two frames of three repeats
    assert e.value.code == -1
    for call in (lambda: coherent.cxavg(rec, X, GOOD, want="mag"), lambda: coherent.process_cxavg(rec, frames, GOOD),
                 lambda: coherent.cxavg_device(rec, 4096, 6, 3, 20, GOOD, 8192, None, None, None),
                 lambda: coherent.process_cxavg_device(rec, 4096, capi.DTYPE_U16, 3, 16, GOOD, None, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = None
