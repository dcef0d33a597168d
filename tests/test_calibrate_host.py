"""CPU tests of the calibration stage's boundary (include/fdoct_calibrate.h): the exports, the function-try-block at every entry
point, the header as C99, the refusals that need no device -- a NULL handle with any arguments, and (where a handle can exist)
a bad slot, nframes < 1, a pitch that is no multiple of 8, width < 1 -- and the argument checks of the Python binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fdoct_amd
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calibrate_header_is_exported_and_listed_and_disjoint_from_the_other_headers():
    """The stage is an add-on library, libfdoct_calibrate.so, over the core library: it exports exactly the header's symbols, the
    core library exports none of them, and load_library attaches them to the object it returns."""
    declared = _declared("fdoct_calibrate.h")
    nm = lambda path: set(re.findall(r"\bT (fdoct_\w+)$", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True), re.M))  # noqa: E731
    assert nm(capi.calibrate_library_path()) == set(declared)
    assert not nm(fdoct_amd.library_path()) & set(declared)
    assert os.path.dirname(capi.calibrate_library_path()) == os.path.dirname(fdoct_amd.library_path())
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(capi.CALIBRATE_ABI_SYMBOLS) == declared and len(declared) == 5
    others = (capi.ABI_SYMBOLS + capi.ROI_ABI_SYMBOLS + capi.CAPTURE_ABI_SYMBOLS + capi.LOWPASS_ABI_SYMBOLS + capi.BSCANBIN_ABI_SYMBOLS +
              capi.COLOUR_ABI_SYMBOLS + capi.MANUALAVG_ABI_SYMBOLS + capi.SAVEFRAMES_ABI_SYMBOLS)
    assert not set(declared) & set(others)
    assert sorted(capi.ABI_SYMBOLS) == _declared("fdoct.h")                 # fdoct.h is what it was
    assert sorted(capi.CAPTURE_ABI_SYMBOLS) == _declared("fdoct_capture.h")  # ... and so is the capture's header


def test_every_calibrate_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_calibrate.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.CALIBRATE_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_calibrate_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_calibrate.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_capture.h"
#include "fdoct_calibrate.h"
int main(void) {
  int held[3] = {7, 7, 7};
  fdoct_cal_slot s = FDOCT_CAL_SAMPLE;
  int (*nrm)(fdoct_handle, const double*, fdoct_memspace, int, int, size_t, double, double, int, double*, fdoct_memspace) =
      fdoct_normalize_rows_minmax;
  int (*cap)(fdoct_handle, int, const void*, fdoct_dtype, fdoct_memspace, int, size_t, double*) = fdoct_calibrate_capture;
  int (*cmp)(fdoct_handle, double*) = fdoct_calibrate_compose;
  int (*clr)(fdoct_handle) = fdoct_calibrate_clear;
  (void)nrm; (void)cap; (void)cmp; (void)clr;
  return (fdoct_calibrate_state(NULL, held) == FDOCT_ERR_INVALID && held[0] == 7 && s == 2 && FDOCT_CAL_DARK == 0 &&
          FDOCT_CAL_REFERENCE == 1) ? 0 : 1;
}
""")
    exe = tmp_path / "use_calibrate"
    libdir = os.path.dirname(fdoct_amd.library_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfdoct_calibrate", "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_null_handle_is_refused_by_every_entry_point_and_touches_nothing():
    lib = fdoct_amd.load_library()
    frames = np.full(64, 9, np.uint16)
    y = np.arange(64, dtype=np.float64)
    out = np.full(64, -7.0)
    held = (C.c_int * 3)(5, 5, 5)
    assert lib.fdoct_normalize_rows_minmax(None, y.ctypes.data, 0, 8, 8, 0, 0.0001, 1.0, 1, out.ctypes.data, 0) == -1
    assert lib.fdoct_normalize_rows_minmax(None, y.ctypes.data, 0, 8, 0, 0, 0.0001, 1.0, 1, out.ctypes.data, 0) == -1     # width < 1
    assert lib.fdoct_normalize_rows_minmax(None, y.ctypes.data, 0, 2, 8, 68, 0.0001, 1.0, 0, out.ctypes.data, 0) == -1    # pitch % 8
    for slot in (0, 1, 2, -1, 3, 99):
        assert lib.fdoct_calibrate_capture(None, slot, frames.ctypes.data, capi.DTYPE_U16, 0, 1, 0, out.ctypes.data) == -1
    assert lib.fdoct_calibrate_capture(None, 0, frames.ctypes.data, capi.DTYPE_U16, 0, 0, 0, out.ctypes.data) == -1       # nframes < 1
    assert lib.fdoct_calibrate_compose(None, out.ctypes.data) == -1
    assert lib.fdoct_calibrate_state(None, held) == -1
    assert lib.fdoct_calibrate_clear(None) == -1
    assert np.all(out == -7.0) and list(held) == [5, 5, 5] and np.array_equal(y, np.arange(64))


def _unbound():
    """A Reconstructor without a handle: the binding's own argument checks raise before the library is reached, and a call that
    gets as far as the library is refused there (NULL handle)."""
    rec = capi.Reconstructor.__new__(capi.Reconstructor)
    rec.lib, rec.h, rec.cfg = fdoct_amd.load_library(), None, fdoct_amd.Config(width=8, height=4, numfftpoints=256, numdisplaypoints=128)
    return rec


def test_binding_checks_its_arguments():
    rec = _unbound()
    y = np.arange(32, dtype=np.float64).reshape(4, 8)
    for bad in (y.astype(np.float32), np.zeros((2, 2, 2)), np.zeros((0, 8)), y[:, ::2]):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.normalize_rows_minmax(bad, out=bad)
        assert e.value.code == -1 and "float64 rows" in str(e.value)
    for out in (np.zeros((4, 8), np.float32), np.zeros((4, 9)), np.zeros((4, 16))[:, :8]):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.normalize_rows_minmax(y, out=out)
        assert e.value.code == -1 and "out must be" in str(e.value)
    frames = np.zeros((1, 4, 8), np.uint16)
    for slot in (-1, 3, None):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.calibrate_capture(slot, frames)
        assert e.value.code == -1 and "slot" in str(e.value)
        with pytest.raises(fdoct_amd.FdoctError) as e:
            rec.calibrate_capture_device(slot, 4096, capi.DTYPE_U16, 1)
        assert e.value.code == -1 and "slot" in str(e.value)
    # what passes the binding's checks reaches the library, which refuses the NULL handle
    for call in (lambda: rec.normalize_rows_minmax(y), lambda: rec.calibrate_capture(capi.CAL_DARK, frames),
                 lambda: rec.calibrate_compose(), lambda: rec.calibrate_state(), lambda: rec.calibrate_clear()):
        with pytest.raises(fdoct_amd.FdoctError) as e:
            call()
        assert e.value.code == -1
    rec.h = None
    assert (fdoct_amd.CAL_DARK, fdoct_amd.CAL_REFERENCE, fdoct_amd.CAL_SAMPLE) == (0, 1, 2)


def test_refusals_on_a_handle_leave_outputs_and_state_untouched():
    """Needs a handle, so a device: without one, creating the handle is the refusal (there is nothing to compute on)."""
    import torch
    cfg = fdoct_amd.Config(width=8, height=4, numfftpoints=256, numdisplaypoints=128)
    if not torch.cuda.is_available():
        with pytest.raises(fdoct_amd.FdoctError) as e:
            fdoct_amd.Reconstructor(cfg)
        assert e.value.code == -3
        return
    rec = fdoct_amd.Reconstructor(cfg)
    lib, h = rec.lib, rec.h
    frames = np.full((1, 4, 8), 9, np.uint16)
    y = np.arange(32, dtype=np.float64)
    out = np.full(32, -7.0)
    nrm = lambda rows, width, pitch, src=y.ctypes.data, dst=out.ctypes.data, space=0: lib.fdoct_normalize_rows_minmax(  # noqa: E731
        h, src, space, rows, width, pitch, 0.0001, 1.0, 1, dst, 0)
    assert nrm(4, 0, 0) == -1 and nrm(0, 8, 0) == -1 and nrm(4, -1, 0) == -1                     # width < 1, rows < 1
    assert nrm(2, 8, 68) == -1 and b"8 bytes" in lib.fdoct_last_error(h)                          # pitch no multiple of 8
    assert nrm(2, 8, 56) == -1 and b"pitch smaller" in lib.fdoct_last_error(h)
    assert nrm(4, 8, 0, src=y.ctypes.data + 4) == -1 and nrm(4, 8, 0, dst=out.ctypes.data + 4) == -1   # pointers aligned to 8 bytes
    assert nrm(4, 8, 0, src=None) == -1 and nrm(4, 8, 0, dst=None) == -1 and nrm(4, 8, 0, space=7) == -1
    assert nrm(2, 8, 0, src=out.ctypes.data, dst=out.ctypes.data + 64) == -1 and b"overlap" in lib.fdoct_last_error(h)
    cap = lambda slot, n=1, dt=capi.DTYPE_U16, p=frames.ctypes.data, pitch=0: lib.fdoct_calibrate_capture(  # noqa: E731
        h, slot, p, dt, 0, n, pitch, out.ctypes.data)
    assert cap(-1) == -1 and b"bad slot" in lib.fdoct_last_error(h)
    assert cap(3) == -1 and cap(0, n=0) == -1 and cap(0, n=-2) == -1 and cap(1, dt=9) == -1 and cap(2, p=None) == -1
    assert cap(0, pitch=14) == -1                                                                 # smaller than a row
    assert lib.fdoct_calibrate_compose(h, out.ctypes.data) == -5 and b"must all be held" in lib.fdoct_last_error(h)   # FDOCT_ERR_STATE
    assert lib.fdoct_calibrate_state(h, None) == -1
    assert np.all(out == -7.0) and rec.calibrate_state() == (False, False, False)
    assert rec.get_reference(capi.REF_DARK) is None and rec.get_reference(capi.REF_BACKGROUND) is None
    rec.close()
