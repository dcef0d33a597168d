"""CPU tests of the colour front end's boundary (include/fdoct_colour.h): the exports, the function-try-block at every entry
point, the constant, and error codes instead of crashes without a device or with bad arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import colour_model
import fdoct_amd
from fdoct_amd import capi
from test_capture_host import _declared, _definitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


def test_colour_header_is_exported_and_listed_and_disjoint_from_the_other_headers():
    declared = _declared("fdoct_colour.h")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", fdoct_amd.library_path()], text=True)
    exported = sorted(s for s in re.findall(r"\bT (fdoct_\w+)$", nm, re.M) if "colour" in s)
    assert declared == exported == sorted(capi.COLOUR_ABI_SYMBOLS) and len(declared) == 4
    assert not [s for s in declared if s.startswith("fdoct_bscan")]
    others = [capi.ABI_SYMBOLS, capi.ROI_ABI_SYMBOLS, capi.CAPTURE_ABI_SYMBOLS, capi.LOWPASS_ABI_SYMBOLS, capi.BSCANBIN_ABI_SYMBOLS]
    for other in others:
        assert not set(declared) & set(other)
    assert sorted(capi.ABI_SYMBOLS) == _declared("fdoct.h") and len(capi.ABI_SYMBOLS) == 50
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name)


def test_every_colour_entry_point_catches_at_the_boundary():
    defs = _definitions(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_colour.cpp"))
    names = [d[0] for d in defs]
    assert len(names) == len(set(names)) and set(names) == set(capi.COLOUR_ABI_SYMBOLS)
    for name, head, tail in defs:
        assert re.search(r"\)\s*try\s*$", head), name + " is not a function-try-block"
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"


def test_colour_header_compiles_as_c99_with_fdoct_h(tmp_path):
    src = tmp_path / "use_colour.c"
    src.write_text("""
#include <stddef.h>
#include "fdoct.h"
#include "fdoct_colour.h"
int main(void) {
  int (*set)(fdoct_handle, int) = fdoct_set_colour_input;
  int (*get)(fdoct_handle, int*) = fdoct_get_colour_input;
  int (*ex)(fdoct_handle, const void*, fdoct_memspace, int, int, int, size_t, int, int, int, int, void*, fdoct_memspace) = fdoct_colour_extract;
  (void)set; (void)get; (void)ex;
  return fdoct_colour_sum_scale() > 0.0 ? 0 : 1;
}
""")
    obj = tmp_path / "use_colour.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    assert obj.exists()


def test_the_sum_scale_is_the_reference_literal():
    assert capi.colour_sum_scale() == 0.00130718954 == colour_model.SUM_SCALE
    assert capi.colour_sum_scale() != 1.0 / 765.0


def test_colour_entry_points_return_codes_for_bad_arguments_without_a_device():
    lib = fdoct_amd.load_library()
    bgr = np.zeros((8, 16, 3), np.uint8)
    out = np.zeros((8, 16), np.float64)
    c = C.c_int(7)
    # a NULL handle
    assert lib.fdoct_set_colour_input(None, 0) == INVALID
    assert lib.fdoct_set_colour_input(None, 4) == INVALID and lib.fdoct_set_colour_input(None, -2) == INVALID
    assert lib.fdoct_get_colour_input(None, C.byref(c)) == INVALID and c.value == 7
    assert lib.fdoct_get_colour_input(None, None) == INVALID

    def extract(bgr_p=bgr.ctypes.data, space=0, n=1, w=16, h=8, pitch=0, ch=0, med=0, bx=1, by=1, out_p=out.ctypes.data, out_space=0):
        return lib.fdoct_colour_extract(None, bgr_p, space, n, w, h, pitch, ch, med, bx, by, out_p, out_space)

    assert extract() == INVALID                      # valid arguments, no handle
    assert extract(bgr_p=None) == INVALID and extract(out_p=None) == INVALID
    assert extract(space=2) == INVALID and extract(out_space=-1) == INVALID
    assert extract(n=0) == INVALID and extract(w=0) == INVALID and extract(h=0) == INVALID and extract(h=-8) == INVALID
    assert extract(ch=4) == INVALID and extract(ch=-2) == INVALID and extract(ch=-1) == INVALID
    assert extract(med=4) == INVALID and extract(med=9) == INVALID
    assert extract(bx=0) == INVALID and extract(by=0) == INVALID
    assert extract(bx=3) == INVALID and extract(by=3) == INVALID and extract(bx=32) == INVALID   # sizes the factors do not divide
    assert extract(pitch=47) == INVALID              # smaller than 3 * raw_w
    # the sum with a median: valid in no reference program, refused as unsupported before the handle is looked at
    assert extract(ch=3, med=3) == UNSUPPORTED and extract(ch=3, med=7, bx=2, by=2) == UNSUPPORTED
    assert b"medianBlur" in lib.fdoct_last_error(None)
    assert extract(ch=3) == INVALID                  # ... and without the median only the handle is missing
