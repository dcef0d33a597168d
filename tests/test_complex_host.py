"""CPU tests of the complex A-scan's boundary (include/fdoct_complex.h): libfdoct_complex.so exports exactly the header's symbols
and the other two libraries none of them, the entry point is a function-try-block, the header compiles as C99 next to fdoct.h,
a NULL handle is refused with the output untouched, the binding checks its arguments, and the wave-per-row kernel's device source
compiles for gfx950 with the option bit that makes it write (re, im) pairs -- alone, with complex rows and with the mirror above
numfftpoints / 2 -- on the shapes the GPU tests run it on, and with the option masks, sample types and depth classes that
tests/test_gpu_complex_options.py adds on that route."""
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_PI, OPT_DARK, OPT_BANDPASS, OPT_ROWNORM, OPT_FRAMENORM, OPT_CPLX, OPT_DEEP, OPT_CXOUT = 1, 2, 4, 8, 16, 64, 128, 256   # FDOCT_WAVE_OPT_* (fdoct_wave.h)


def _exports(path):
    return set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))


def test_complex_header_is_exported_by_its_own_library_only():
    declared = _declared("fdoct_complex.h")
    assert declared == ["fdoct_process_complex"] == sorted(capi.COMPLEX_ABI_SYMBOLS)
    assert _exports(capi.complex_library_path()) == set(declared)
    assert not _exports(fdoct_amd.library_path()) & set(declared)
    assert not _exports(capi.calibrate_library_path()) & set(declared)
    assert os.path.dirname(capi.complex_library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    assert hasattr(lib, "fdoct_process_complex")
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS + capi.CALIBRATE_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    assert sorted(capi.ABI_SYMBOLS) == _declared("fdoct.h")   # fdoct.h is what it was
    # the function the entry point calls in the core library has C++ linkage: no exported fdoct_ name
    core = subprocess.check_output(["nm", "-D", "--defined-only", fdoct_amd.library_path()], text=True)
    assert re.search(r"\bT _ZN10fdoct_impl15enqueue_complexE", core)


def test_the_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_complex.cpp"))
    assert [d[0] for d in defs] == capi.COMPLEX_ABI_SYMBOLS
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_complex_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_complex.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_complex.h"
int main(void) {
  float out[4] = {7.f, 7.f, 7.f, 7.f};
  unsigned short frames[4] = {1, 2, 3, 4};
  int (*cx)(fdoct_handle, const void*, fdoct_dtype, fdoct_memspace, int, size_t, float*, fdoct_memspace, fdoct_layout) = fdoct_process_complex;
  return (cx(NULL, frames, FDOCT_U16, FDOCT_MEM_HOST, 1, 0, out, FDOCT_MEM_HOST, FDOCT_LAYOUT_ROWMAJOR_HxD) == FDOCT_ERR_INVALID &&
          out[0] == 7.f && out[3] == 7.f) ? 0 : 1;
}
""")
    exe = tmp_path / "use_complex"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_complex", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_null_handle_is_refused_and_touches_nothing():
    lib = fdoct_amd.load_library()
    frames = np.full(64, 9, np.uint16)
    out = np.full(64, -7.0, np.float32)
    for layout in (capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED, 5):
        for space in (capi.MEM_HOST, capi.MEM_DEVICE, 9):
            assert lib.fdoct_process_complex(None, frames.ctypes.data, capi.DTYPE_U16, space, 1, 0, out.ctypes.data, space, layout) == -1
    assert lib.fdoct_process_complex(None, None, capi.DTYPE_U16, 0, 1, 0, None, 0, 0) == -1
    assert np.all(out == -7.0) and np.all(frames == 9)


def test_binding_checks_its_arguments():
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=256, numdisplaypoints=128)
    frames = np.zeros((2, 4, 8), np.uint16)
    with pytest.raises(fdoct_amd.FdoctError) as e:
        rec.process_complex(frames.astype(np.int64))
    assert e.value.code == -1 and "dtype" in str(e.value)
    for out in (np.zeros((2, 4, 128), np.complex128), np.zeros((2, 128, 4), np.complex64), np.zeros((2, 4, 256), np.complex64)[:, :, ::2]):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.process_complex(frames, out=out)
        assert e.value.code == -1 and "complex64" in str(e.value)
    good = np.full((2, 128, 4), 3 - 4j, np.complex64)
    for call in (lambda: rec.process_complex(frames, layout=capi.LAYOUT_TRANSPOSED, out=good),
                 lambda: rec.process_complex_device(4096, capi.DTYPE_U16, 2, 16, 8192)):
        with pytest.raises(fdoct_amd.FdoctError) as e:   # what passes the binding's checks reaches the library, which refuses the NULL handle
            call()
        assert e.value.code == -1
    assert np.all(good == np.complex64(3 - 4j))
    rec.h = None


# (W, M, N, D, dtype, option mask next to FDOCT_WAVE_OPT_CXOUT): the shapes of tests/test_gpu_complex.py's wave route
JIT_CASES = [
    ("200 x4 -> 2560, D 320", 200, 4, 2560, 320, capi.DTYPE_U16, 0),
    ("2048 -> 2048, D 1024", 2048, 1, 2048, 1024, capi.DTYPE_U16, 0),
    ("2048 -> 2048, D 1024, complex rows", 2048, 1, 2048, 1024, capi.DTYPE_U16, OPT_CPLX),
    ("640 -> 640, D 640, mirror", 640, 1, 640, 640, capi.DTYPE_U8, OPT_DEEP),
    ("200 x4 -> 2560, D 320, pi + dark + whole-frame normalisation", 200, 4, 2560, 320, capi.DTYPE_U16, OPT_PI | OPT_DARK | OPT_FRAMENORM),
    # ... and the option masks and shapes tests/test_gpu_complex_options.py adds on that route
    ("200 x4 -> 2560, D 320, band-pass", 200, 4, 2560, 320, capi.DTYPE_U16, OPT_BANDPASS),
    ("200 x4 -> 2560, D 320, row-wise normalisation", 200, 4, 2560, 320, capi.DTYPE_U16, OPT_ROWNORM),
    ("200 x4 -> 2560, D 320, band-pass + row-wise normalisation + pi + dark", 200, 4, 2560, 320, capi.DTYPE_U16, OPT_BANDPASS | OPT_ROWNORM | OPT_PI | OPT_DARK),
    ("160 x4 -> 2560, D 320, complex rows", 160, 4, 2560, 320, capi.DTYPE_U16, OPT_CPLX),
    ("640 -> 640, D 640, complex rows", 640, 1, 640, 640, capi.DTYPE_U16, OPT_CPLX),
    ("1280 x4 -> 2560, D 320", 1280, 4, 2560, 320, capi.DTYPE_U16, 0),
    ("640 x4 -> 2560, D 320", 640, 4, 2560, 320, capi.DTYPE_U16, 0),
    ("200 x4 -> 2560, D 320, f32 frames", 200, 4, 2560, 320, capi.DTYPE_F32, 0),
    ("640 -> 640, D 1", 640, 1, 640, 1, capi.DTYPE_U16, 0),
    ("640 -> 640, D 321, mirror (bin N/2 alone)", 640, 1, 640, 321, capi.DTYPE_U16, OPT_DEEP),
    ("200 x4 -> 2560, D 2560, mirror", 200, 4, 2560, 2560, capi.DTYPE_U16, OPT_DEEP),
]


@pytest.mark.parametrize("case", JIT_CASES, ids=[c[0] for c in JIT_CASES])
def test_the_wave_kernel_compiles_with_the_complex_output_option(case, monkeypatch):
    _, W, M, N, D, dt, opt = case
    monkeypatch.setenv("FDOCT_JIT_CHECK_OPT", str(OPT_CXOUT | opt))
    nbytes, why = capi.jit_compile_check(W, M, N, D, dtype=dt)
    if nbytes <= 0 and "libhiprtc" in why:
        pytest.skip("run-time compiler not available: " + why)
    assert nbytes > 0, why
