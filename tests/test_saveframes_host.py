"""CPU tests of the boundary of include/fdoct_saveframes.h on the built library, without a device: the exports, the
function-try-block at every entry point, both headers as C99, the version that follows the header, and error codes instead of
crashes for every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fdoct_amd
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
HXD, DXH = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED


def test_saveframes_header_is_exported_and_listed_and_on_its_own():
    declared = _declared("fdoct_saveframes.h")
    assert declared == sorted(capi.SAVEFRAMES_ABI_SYMBOLS) == ["fdoct_get_raw_magnitudes", "fdoct_saveframes", "fdoct_set_raw_magnitudes"]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", fdoct_amd.library_path()], text=True)
    exported = set(re.findall(r"\bT (fdoct_\w+)$", nm, re.M))
    assert set(declared) <= exported
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)
    others = [capi.ABI_SYMBOLS, capi.ROI_ABI_SYMBOLS, capi.CAPTURE_ABI_SYMBOLS, capi.LOWPASS_ABI_SYMBOLS, capi.BSCANBIN_ABI_SYMBOLS,
              capi.COLOUR_ABI_SYMBOLS, capi.MANUALAVG_ABI_SYMBOLS]
    for other in others:
        assert not set(declared) & set(other)
    # every exported fdoct_ symbol is declared by one of the headers
    assert exported == set(declared).union(*others)
    assert sorted(capi.ABI_SYMBOLS) == _declared("fdoct.h")


def test_every_saveframes_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_saveframes.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.SAVEFRAMES_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_version_follows_the_header():
    hdr = open(os.path.join(ROOT, "include", "fdoct.h")).read()
    major = int(re.search(r"#define FDOCT_VERSION_MAJOR (\d+)", hdr).group(1))
    minor = int(re.search(r"#define FDOCT_VERSION_MINOR (\d+)", hdr).group(1))
    assert (major, minor) == (0, 5)
    assert fdoct_amd.load_library().fdoct_version().decode().split()[1] == "%d.%d" % (major, minor)


def test_both_headers_compile_as_c99(tmp_path):
    src = tmp_path / "use_saveframes.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_saveframes.h"
int main(void) {
  int (*set)(fdoct_handle, int) = fdoct_set_raw_magnitudes;
  int (*get)(fdoct_handle) = fdoct_get_raw_magnitudes;
  int (*save)(fdoct_handle, const float*, fdoct_memspace, fdoct_layout, int, int, int, unsigned char*, int, float*, float*,
              fdoct_layout, fdoct_memspace) = fdoct_saveframes;
  (void)set; (void)get; (void)save;
  return FDOCT_VERSION_MINOR >= 5 ? 0 : 1;
}
""")
    obj = tmp_path / "use_saveframes.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    assert obj.exists()
    only = tmp_path / "only_fdoct.c"
    only.write_text('#include "fdoct.h"\nint main(void) { return FDOCT_VERSION_MAJOR; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(only),
                           "-o", str(tmp_path / "only_fdoct.o")])


def test_refusals_that_need_no_device():
    lib = fdoct_amd.load_library()
    src = np.full(2 * 12, 3.0, np.float32)
    gray = np.full(2 * 12, 0xA5, np.uint8)
    mag, db = np.full(2 * 12, -7.0, np.float32), np.full(2 * 12, -7.0, np.float32)

    def call(h=None, frames=src.ctypes.data, mem=HOST, il=HXD, n=2, d=4, a=3, g=gray.ctypes.data, avg=1, b=mag.ctypes.data,
             o=db.ctypes.data, ol=DXH, om=HOST):
        return lib.fdoct_saveframes(h, frames, mem, il, n, d, a, g, avg, b, o, ol, om)

    assert call() == INVALID                                         # a correct call but for its handle
    assert lib.fdoct_set_raw_magnitudes(None, 1) == INVALID and lib.fdoct_get_raw_magnitudes(None) == INVALID
    for bad in (dict(frames=None), dict(mem=2), dict(mem=-1), dict(om=2), dict(il=2), dict(il=-1), dict(ol=2), dict(n=0), dict(n=-2),
                dict(d=0), dict(a=0), dict(avg=-1)):
        assert call(**bad) == INVALID, bad
        assert b"fdoct_saveframes: bad arguments" in lib.fdoct_last_error(None), bad
    assert call(n=2, avg=3) == INVALID and b"multiple of averages" in lib.fdoct_last_error(None)
    assert call(g=None, b=None, o=None) == INVALID and b"no output" in lib.fdoct_last_error(None)
    assert call(avg=0) == INVALID and b"averages = 0" in lib.fdoct_last_error(None)
    assert call(avg=0, b=None) == INVALID and call(avg=0, o=None) == INVALID
    assert call(d=1 << 30, a=1 << 30) == INVALID and b"too large" in lib.fdoct_last_error(None)
    assert (gray == 0xA5).all() and (mag == -7.0).all() and (db == -7.0).all() and (src == 3.0).all()
