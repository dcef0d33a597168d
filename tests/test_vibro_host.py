"""CPU tests of the vibrometry stage's boundary (include/fdoct_vibro.h): libfdoct_vibro.so exports exactly the header's symbols and
the other five libraries none of them, the entry points are function-try-blocks, the header compiles as C99 next to fdoct.h, the
ctypes mirrors have the structs' layout, a NULL handle is refused with the outputs untouched, fdoct_vibro_plan's refusals and
geometry, and the binding checks its arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
from fdoct_amd import capi, dispersion, vibrometry
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_vibro_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_vibro.h")
    assert declared == sorted(vibrometry.VIBRO_ABI_SYMBOLS) == ["fdoct_process_vibro", "fdoct_vibro", "fdoct_vibro_plan"]
    assert _exports(vibrometry.library_path()) == set(declared)
    for other in (fdoct_amd.library_path(), capi.calibrate_library_path(), capi.complex_library_path(), capi.doppler_library_path(),
                  dispersion.library_path()):
        assert not _exports(other) & set(declared), other
    assert os.path.dirname(vibrometry.library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS + capi.COMPLEX_ABI_SYMBOLS +
              capi.DOPPLER_ABI_SYMBOLS + dispersion.DISPERSION_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    needed = subprocess.check_output(["readelf", "-d", vibrometry.library_path()], text=True)
    assert "libfdoct_hip.so" in needed and "$ORIGIN" in needed
    # functions over a Reconstructor, not methods of it
    for name in ("library_path", "params", "plan", "vibro", "vibro_device", "process_vibro", "process_vibro_device"):
        assert callable(getattr(vibrometry, name)) and not hasattr(capi.Reconstructor, name)


def test_the_entry_points_catch_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_vibro.cpp"))
    assert [d[0] for d in defs] == vibrometry.VIBRO_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_vibro_header_compiles_as_c99_and_the_mirrors_have_its_layout(tmp_path):
    src = tmp_path / "use_vibro.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "fdoct.h"
#include "fdoct_vibro.h"
int main(void) {
  float x[2 * 4 * 3 * 5], out[4] = {7.f, 7.f, 7.f, 7.f};
  unsigned short frames[4] = {1, 2, 3, 4};
  fdoct_vibro_params p = {1, 1, 2, 1, FDOCT_VIBRO_HANN, 2, {0.25, 0.5, 0, 0, 0, 0, 0, 0}, 2.0, 0.0, 2};
  fdoct_vibro_info info;
  int i;
  for (i = 0; i < 120; i++) x[i] = 1.f;
  if (fdoct_vibro_plan(&p, 4, 3, 5, &info) != FDOCT_OK || info.chunk_steps != 2 || info.chunks != 2 || info.workgroups != 2) return 1;
  if (info.workspace_bytes != 4 * 3 * 8 + 2 * 9 * 15 * 8 + (2 * 4 + 2 * 3 * 2 + 9) * 16) return 2;
  info.chunks = -3;
  p.nfreq = 9;
  if (fdoct_vibro_plan(&p, 4, 3, 5, &info) != FDOCT_ERR_INVALID || info.chunks != -3) return 3;
  p.nfreq = 2;
  if (fdoct_vibro(NULL, x, FDOCT_MEM_HOST, 4, 3, 5, &p, NULL, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 4;
  if (fdoct_process_vibro(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 2, 0, &p, NULL, out, NULL, NULL, FDOCT_MEM_HOST) != FDOCT_ERR_INVALID) return 5;
  if (out[0] != 7.f || out[3] != 7.f) return 6;
  printf("%d %d %d %d %d %d %d %d %d %d %d", (int)sizeof(fdoct_vibro_params), (int)offsetof(fdoct_vibro_params, nfreq),
         (int)offsetof(fdoct_vibro_params, freq), (int)offsetof(fdoct_vibro_params, scale), (int)offsetof(fdoct_vibro_params, min_power),
         (int)offsetof(fdoct_vibro_params, chunk_steps), (int)sizeof(fdoct_vibro_info), (int)offsetof(fdoct_vibro_info, chunks),
         (int)offsetof(fdoct_vibro_info, workgroups), (int)offsetof(fdoct_vibro_info, workspace_bytes), FDOCT_VIBRO_MAX_FREQ);
  return 0;
}
""")
    exe = tmp_path / "use_vibro"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_vibro", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    done = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.returncode
    P, I = vibrometry._CParams, vibrometry._CInfo
    assert [int(v) for v in done.stdout.split()] == [C.sizeof(P), P.nfreq.offset, P.freq.offset, P.scale.offset, P.min_power.offset, P.chunk_steps.offset,
                                                     C.sizeof(I), I.chunks.offset, I.workgroups.offset, I.workspace_bytes.offset, vibrometry.MAX_FREQ]
    assert C.sizeof(P) == 112 and C.sizeof(I) == 24 and (vibrometry.RECT, vibrometry.HANN) == (0, 1)


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    X = np.full(4 * 3 * 5, 2 + 1j, np.complex64)
    frames = np.full(64, 9, np.uint16)
    outs = [np.full(256, -7.0, np.float32) for _ in range(4)]
    p = vibrometry.params(freq=(0.25,), ref=True)
    ptrs = [o.ctypes.data for o in outs]
    for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
        assert lib.fdoct_vibro(None, X.ctypes.data, space, 4, 3, 5, p, *ptrs, space) == -1
        assert lib.fdoct_process_vibro(None, frames.ctypes.data, capi.DTYPE_U16, space, 2, 0, p, *ptrs, space) == -1
    assert lib.fdoct_vibro(None, None, 0, 4, 3, 5, None, None, None, None, None, 0) == -1
    assert all(np.all(o == -7.0) for o in outs) and np.all(frames == 9) and np.all(X == np.complex64(2 + 1j))


GOOD = dict(freq=(0.1, 0.5), ref=(2, 3))
# (params' keywords, T, H, D) -> (chunk_steps, chunks, workgroups), or the refusal's code
PLAN_CASES = [
    ((GOOD, 2, 1, 5), (1, 1, 1)), ((GOOD, 6, 3, 20), (5, 1, 1)), ((dict(GOOD, chunk_steps=2), 6, 3, 20), (2, 3, 3)),
    ((dict(GOOD, chunk_steps=99), 6, 3, 20), (5, 1, 1)),                      # more steps than there are: one chunk of them all
    ((GOOD, 65536, 1, 1024), (1024, 64, 256)), ((GOOD, 4096, 1, 1024), (64, 64, 256)), ((GOOD, 64, 1000, 1024), (63, 1, 4000)),
    ((dict(GOOD, chunk_steps=1), 65536, 1, 64), (1, 65535, 65535)),
    ((GOOD, 2, 1 << 12, 1 << 12), (1, 1, 1 << 16)),                           # 2^24 pixels
    ((GOOD, 2, 1 << 12, (1 << 12) + 1), -1), ((GOOD, 2, 1 << 24, 5), -1), ((GOOD, 2, 1 << 16, 1 << 16), -1),
    ((GOOD, 1, 3, 20), -1), ((GOOD, 0, 3, 20), -1), ((GOOD, -5, 3, 20), -1), ((GOOD, 65537, 3, 20), -1),
    ((GOOD, 6, 0, 20), -1), ((GOOD, 6, 3, 0), -1), ((GOOD, 6, -3, 20), -1), ((GOOD, 6, 3, -20), -1),
    ((dict(GOOD, freq=(0.0,)), 6, 3, 20), -1), ((dict(GOOD, freq=(0.51,)), 6, 3, 20), -1), ((dict(GOOD, freq=(-0.25,)), 6, 3, 20), -1),
    ((dict(GOOD, freq=(0.1, float("nan"))), 6, 3, 20), -1), ((dict(GOOD, freq=(float("inf"),)), 6, 3, 20), -1),
    ((dict(GOOD, freq=(0.5,) * 8), 6, 3, 20), (5, 1, 1)), ((dict(GOOD, freq=()), 6, 3, 20), (5, 1, 1)),
    ((dict(GOOD, ref=(0, 0)), 6, 3, 20), (5, 1, 1)), ((dict(GOOD, ref=(19, 1)), 6, 3, 20), (5, 1, 1)), ((dict(GOOD, ref=(0, 20)), 6, 3, 20), (5, 1, 1)),
    ((dict(GOOD, ref=(20, 0)), 6, 3, 20), -1), ((dict(GOOD, ref=(-1, 0)), 6, 3, 20), -1), ((dict(GOOD, ref=(0, 21)), 6, 3, 20), -1),
    ((dict(GOOD, ref=(19, 2)), 6, 3, 20), -1), ((dict(GOOD, ref=(5, -1)), 6, 3, 20), -1),
    ((dict(GOOD, detrend=1, window=1), 6, 3, 20), (5, 1, 1)), ((dict(GOOD, detrend=2), 6, 3, 20), -1), ((dict(GOOD, detrend=-1), 6, 3, 20), -1),
    ((dict(GOOD, window=2), 6, 3, 20), -1), ((dict(GOOD, window=-1), 6, 3, 20), -1),
    ((dict(GOOD, scale=float("nan")), 6, 3, 20), -1), ((dict(GOOD, scale=float("-inf")), 6, 3, 20), -1), ((dict(GOOD, scale=-4.5), 6, 3, 20), (5, 1, 1)),
    ((dict(GOOD, min_power=float("nan")), 6, 3, 20), -1), ((dict(GOOD, min_power=float("inf")), 6, 3, 20), -1), ((dict(GOOD, min_power=-1e-30), 6, 3, 20), -1),
    ((dict(GOOD, chunk_steps=-1), 6, 3, 20), -1),
]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[str(c[0]) for c in PLAN_CASES])
def test_vibro_plan(case):
    (kw, T, H, D), want = case
    if isinstance(want, int):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            vibrometry.plan(kw, T, H, D)
        assert e.value.code == want
    else:
        p = vibrometry.plan(kw, T, H, D)
        assert (p["chunk_steps"], p["chunks"], p["workgroups"]) == want
        nf, n, ref = len(kw["freq"]), want[1], kw["ref"] is not None
        bytes_ = (T * H * 8 if ref else 0) + (n * (5 + 2 * nf) * H * D * 8 if n > 1 else 0) + ((nf * T + n * (nf + 1) * 2 + 3 * (nf + 1)) * 16 if nf else 0)
        assert p["workspace_bytes"] == bytes_


def test_vibro_plan_refuses_missing_pointers_and_bad_counts_and_leaves_its_output_alone():
    lib = fdoct_amd.load_library()
    p, info = vibrometry.params(**GOOD), vibrometry._CInfo(-5, -6, -7, 8)
    assert lib.fdoct_vibro_plan(None, 6, 3, 20, C.byref(info)) == -1
    assert lib.fdoct_vibro_plan(C.byref(p), 6, 3, 20, None) == -1
    for nf in (-1, 9, 1 << 30):
        p.nfreq = nf
        assert lib.fdoct_vibro_plan(C.byref(p), 6, 3, 20, C.byref(info)) == -1
    p.nfreq, p.ref = 2, 2
    assert lib.fdoct_vibro_plan(C.byref(p), 6, 3, 20, C.byref(info)) == -1
    assert (info.chunk_steps, info.chunks, info.workgroups, info.workspace_bytes) == (-5, -6, -7, 8)


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=128, numdisplaypoints=64)
    X = np.zeros((4, 3, 20), np.complex64)
    for bad in (X.astype(np.complex128), X.view(np.float32), np.zeros((4, 60), np.complex64), np.zeros((0, 3, 20), np.complex64)):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            vibrometry.vibro(rec, bad, GOOD)
        assert e.value.code == -1 and "complex64" in str(e.value)
    for kw in (dict(want=()), dict(want=("rms", "phase")), dict(want=("rms", "rms")), dict(want="table")):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            vibrometry.vibro(rec, X, GOOD, **kw)
        assert e.value.code == -1, kw
    for bad in (dict(freq=(0.1,) * 9), dict(freq=("x",)), dict(ref=5), dict(ref=(1, 2, 3)), dict(freq=(0.7,)), dict(ref=(20, 0))):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            vibrometry.vibro(rec, X, dict(GOOD, **bad))
        assert e.value.code == -1, bad
    frames = np.zeros((3, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        vibrometry.process_vibro(rec, frames.astype(np.int64), GOOD)
    assert e.value.code == -1 and "dtype" in str(e.value)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        vibrometry.process_vibro(rec, frames[:1], GOOD)       # one frame: no step
    assert e.value.code == -1
    for call in (lambda: vibrometry.vibro(rec, X, GOOD, want="rms"), lambda: vibrometry.process_vibro(rec, frames, GOOD),
                 lambda: vibrometry.vibro_device(rec, 4096, 4, 3, 20, GOOD, 8192, None, None, None),
                 lambda: vibrometry.process_vibro_device(rec, 4096, capi.DTYPE_U16, 3, 16, GOOD, None, None, 8192, None)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    rec.h = None
