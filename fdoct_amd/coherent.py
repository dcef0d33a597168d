"""The binding of include/fdoct_cxavg.h: coherent averaging of repeated complex B-scans on the GPU -- per group of `repeats`
frames the complex mean after the repeats' common phase is taken out, its modulus, the mean of the moduli over the same frames
and the ratio of the two sums.  The entry points live in libfdoct_cxavg.so, a seventh add-on library over libfdoct_hip.so;
capi.load_library attaches them to the object it returns (attach, below).  Functions over a Reconstructor, not methods of it.

    from fdoct_amd import coherent
    p = coherent.params(repeats=4, align=1)
    out = coherent.process_cxavg(rec, frames, p)     # out["mag"]: (groups, height, depths), frames = groups * 4

Group g's repeat n is frame g * stride + n; stride None means repeats (disjoint groups), a smaller one a sliding average.  align is
0 (none), 1 (a phasor per group, repeat and A-scan) or 2 (per group and repeat); align_range is (first, count), count 0 meaning up
to the last depth."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, FdoctError

# every symbol include/fdoct_cxavg.h declares
CXAVG_ABI_SYMBOLS = ["fdoct_cxavg_plan", "fdoct_cxavg", "fdoct_process_cxavg"]
WANTS = ("mean", "mag", "incoh", "coh")
MAX_REPEATS, REG_PAIRS = 64, 16
FORM_REGISTER, FORM_STREAMING = 1, 2


class _CParams(C.Structure):
    """fdoct_cxavg_params."""
    _fields_ = [("repeats", C.c_int), ("stride", C.c_int), ("ref", C.c_int), ("align", C.c_int), ("align_first", C.c_int), ("align_count", C.c_int)]


class _CInfo(C.Structure):
    """fdoct_cxavg_info."""
    _fields_ = [("groups", C.c_int), ("form", C.c_int), ("workgroups", C.c_longlong), ("workspace_bytes", C.c_size_t)]


def library_path():
    """The add-on library of include/fdoct_cxavg.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_cxavg.so")


def attach(lib):
    """Loads libfdoct_cxavg.so and attaches its entry points to the core library's object (capi.load_library calls this)."""
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % path)
    cxa = C.CDLL(path)
    for name in CXAVG_ABI_SYMBOLS:
        setattr(lib, name, getattr(cxa, name))
    lib.fdoct_cxavg_plan.argtypes = [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(_CInfo)]
    lib.fdoct_cxavg.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_CParams), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_cxavg.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_CParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def params(repeats=2, stride=None, ref=0, align=1, align_range=(0, 0)):
    """fdoct_cxavg_params.  The library, not this function, refuses bad values; what does not fit the structure is refused here."""
    try:
        first, count = align_range
        return _CParams(int(repeats), int(repeats if stride is None else stride), int(ref), int(align), int(first), int(count))
    except (TypeError, ValueError):
        raise FdoctError(-1, "repeats, stride, ref and align are numbers, align_range is (first, count)")


def _params(p):
    return p if isinstance(p, _CParams) else params(**p)


def plan(p, nframes, ascans, depths):
    """fdoct_cxavg_plan: the geometry of a call as a dict (groups, form, workgroups, workspace_bytes), or FdoctError -1 where the
    call would be refused.  Needs no GPU."""
    p, info = _params(p), _CInfo()
    rc = capi.load_library().fdoct_cxavg_plan(C.byref(p), int(nframes), int(ascans), int(depths), C.byref(info))
    if rc:
        raise FdoctError(rc, "fdoct_cxavg_plan: repeats 2..64, stride 1..repeats, frames repeats plus a multiple of stride and at most 65536, "
                             "ref 0..repeats-1, at most 2^24 pixels, align 0..2 with a range inside [0, depths)")
    return {k: int(getattr(info, k)) for k, _ in _CInfo._fields_}


def _outputs(want, groups, ascans, depths):
    if isinstance(want, str):
        want = (want,)
    if want is None:
        want = WANTS
    if not want or any(w not in WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of %s, each once" % (WANTS,))
    return tuple(want), {w: np.empty((groups, ascans, depths), np.complex64 if w == "mean" else np.float32) for w in want}


def _result(want, names, outs):
    return outs[names[0]] if isinstance(want, str) else {w: outs[w] for w in names}


def cxavg(rec, X, p, want=None):
    """fdoct_cxavg on host memory: X is complex64 (nframes, ascans, depths), as process_complex returns it.  Returns a dict of the
    outputs `want` names (one name as a string: that output alone; None: all four), each (groups, ascans, depths): "mean" complex64,
    the others float32.  Synchronous."""
    a = np.asarray(X)
    if a.dtype != np.complex64 or a.ndim != 3 or a.size == 0:
        raise FdoctError(-1, "X must be complex64 of shape (nframes, ascans, depths)")
    a = np.ascontiguousarray(a)
    p = _params(p)
    T, H, D = a.shape
    info = plan(p, T, H, D)
    names, outs = _outputs(want, info["groups"], H, D)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_cxavg(rec.h, a.ctypes.data, MEM_HOST, T, H, D, C.byref(p), ptr("mean"), ptr("mag"), ptr("incoh"), ptr("coh"), MEM_HOST))
    return _result(want, names, outs)


def cxavg_device(rec, d_re_im_ptr, nframes, ascans, depths, p, d_mean_ptr, d_mag_ptr, d_incoh_ptr, d_coh_ptr):
    """... on device-resident pairs into device memory (raw addresses; the pairs and d_mean_ptr aligned to 8 bytes, the other
    outputs to 4; any output may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_cxavg(rec.h, d_re_im_ptr, MEM_DEVICE, int(nframes), int(ascans), int(depths), C.byref(p), d_mean_ptr, d_mag_ptr,
                                   d_incoh_ptr, d_coh_ptr, MEM_DEVICE))


def process_cxavg(rec, frames, p, want=None):
    """fdoct_process_cxavg: process_complex's chain on `frames` (numpy, as process() takes them) followed by cxavg() on the card,
    ascans = height and depths = numdisplaypoints; the complex A-scans never reach the host.  The handle must have `averages` 1.
    Returns what cxavg() returns.  Synchronous."""
    a = np.ascontiguousarray(frames)
    if a.ndim == 2:
        a = a[None]
    if a.dtype not in capi._NP2DT:
        raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
    if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
        raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
    p = _params(p)
    T, H, D = a.shape[0], rec.cfg.height, rec.cfg.numdisplaypoints
    info = plan(p, T, H, D)
    names, outs = _outputs(want, info["groups"], H, D)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_process_cxavg(rec.h, a.ctypes.data, capi._NP2DT[a.dtype], MEM_HOST, T, a.strides[1], C.byref(p), ptr("mean"), ptr("mag"),
                                           ptr("incoh"), ptr("coh"), MEM_HOST))
    return _result(want, names, outs)


def process_cxavg_device(rec, d_frames_ptr, dtype, nframes, pitch_bytes, p, d_mean_ptr, d_mag_ptr, d_incoh_ptr, d_coh_ptr):
    """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_process_cxavg(rec.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), C.byref(p), d_mean_ptr, d_mag_ptr,
                                           d_incoh_ptr, d_coh_ptr, MEM_DEVICE))
