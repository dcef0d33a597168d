"""The binding of include/fdoct_angio.h: OCT angiography from repeated B-scans on the GPU -- per slow-axis position the speckle
variance of the intensity, the amplitude decorrelation, the complex decorrelation with bulk-motion correction and the mean power
of its `repeats` complex B-scans.  The entry points live in libfdoct_angio.so, a sixth add-on library over libfdoct_hip.so;
capi.load_library attaches them to the object it returns (attach, below).  Functions over a Reconstructor, not methods of it.

    from fdoct_amd import angiography
    p = angiography.params(repeats=4, win=(3, 5), bulk=True)
    out = angiography.process_angio(rec, frames, p)     # out["cdecorr"]: (positions, height, depths), frames = positions * 4

Frame g * repeats + n is repeat n of position g.  win is (A-scans, depths), each 1 .. 16.  bulk is None, True (every depth) or
(first, count), count 0 meaning up to the last depth."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, FdoctError

# every symbol include/fdoct_angio.h declares
ANGIO_ABI_SYMBOLS = ["fdoct_angio_plan", "fdoct_angio", "fdoct_process_angio"]
WANTS = ("var", "decorr", "cdecorr", "power")
MAX_WIN, MAX_REPEATS = 16, 64


class _CParams(C.Structure):
    """fdoct_angio_params."""
    _fields_ = [("repeats", C.c_int), ("win_ascans", C.c_int), ("win_depths", C.c_int), ("bulk", C.c_int), ("bulk_first", C.c_int),
                ("bulk_count", C.c_int), ("min_power", C.c_double)]


class _CInfo(C.Structure):
    """fdoct_angio_info."""
    _fields_ = [("groups", C.c_int), ("tiles", C.c_longlong), ("workgroups", C.c_longlong), ("workspace_bytes", C.c_size_t)]


def library_path():
    """The add-on library of include/fdoct_angio.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_angio.so")


def attach(lib):
    """Loads libfdoct_angio.so and attaches its entry points to the core library's object (capi.load_library calls this)."""
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % path)
    ang = C.CDLL(path)
    for name in ANGIO_ABI_SYMBOLS:
        setattr(lib, name, getattr(ang, name))
    lib.fdoct_angio_plan.argtypes = [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(_CInfo)]
    lib.fdoct_angio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_CParams), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_angio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_CParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def params(repeats=2, win=(1, 1), bulk=None, min_power=0.0):
    """fdoct_angio_params.  The library, not this function, refuses bad values; what does not fit the structure is refused here."""
    try:
        wa, wd = win
        if bulk is None or bulk is False:
            use, first, count = 0, 0, 0
        else:
            use, (first, count) = 1, ((0, 0) if bulk is True else bulk)
        return _CParams(int(repeats), int(wa), int(wd), use, int(first), int(count), float(min_power))
    except (TypeError, ValueError):
        raise FdoctError(-1, "repeats is a number, win is (A-scans, depths), bulk is None, True or (first, count)")


def _params(p):
    return p if isinstance(p, _CParams) else params(**p)


def plan(p, nframes, ascans, depths):
    """fdoct_angio_plan: the geometry of a call as a dict (groups, tiles, workgroups, workspace_bytes), or FdoctError -1 where the
    call would be refused.  Needs no GPU."""
    p, info = _params(p), _CInfo()
    rc = capi.load_library().fdoct_angio_plan(C.byref(p), int(nframes), int(ascans), int(depths), C.byref(info))
    if rc:
        raise FdoctError(rc, "fdoct_angio_plan: repeats 2..64, frames a positive multiple of repeats and at most 65536, at most 2^24 pixels, "
                             "windows 1..16, bulk 0 or 1 with a range inside [0, depths), finite min_power >= 0")
    return {k: int(getattr(info, k)) for k, _ in _CInfo._fields_}


def _outputs(want, groups, ascans, depths):
    if isinstance(want, str):
        want = (want,)
    if want is None:
        want = WANTS
    if not want or any(w not in WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of %s, each once" % (WANTS,))
    return tuple(want), {w: np.empty((groups, ascans, depths), np.float32) for w in want}


def _result(want, names, outs):
    return outs[names[0]] if isinstance(want, str) else {w: outs[w] for w in names}


def angio(rec, X, p, want=None):
    """fdoct_angio on host memory: X is complex64 (nframes, ascans, depths), as process_complex returns it, nframes = groups *
    repeats.  Returns a dict of the outputs `want` names (one name as a string: that output alone; None: all four), each
    (groups, ascans, depths) float32.  Synchronous."""
    a = np.asarray(X)
    if a.dtype != np.complex64 or a.ndim != 3 or a.size == 0:
        raise FdoctError(-1, "X must be complex64 of shape (nframes, ascans, depths)")
    a = np.ascontiguousarray(a)
    p = _params(p)
    T, H, D = a.shape
    info = plan(p, T, H, D)
    names, outs = _outputs(want, info["groups"], H, D)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_angio(rec.h, a.ctypes.data, MEM_HOST, T, H, D, C.byref(p), ptr("var"), ptr("decorr"), ptr("cdecorr"), ptr("power"), MEM_HOST))
    return _result(want, names, outs)


def angio_device(rec, d_re_im_ptr, nframes, ascans, depths, p, d_var_ptr, d_decorr_ptr, d_cdecorr_ptr, d_power_ptr):
    """... on device-resident pairs into device memory (raw addresses; the pairs aligned to 8 bytes, the outputs to 4; any output
    may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_angio(rec.h, d_re_im_ptr, MEM_DEVICE, int(nframes), int(ascans), int(depths), C.byref(p), d_var_ptr, d_decorr_ptr,
                                   d_cdecorr_ptr, d_power_ptr, MEM_DEVICE))


def process_angio(rec, frames, p, want=None):
    """fdoct_process_angio: process_complex's chain on `frames` (numpy, as process() takes them; frame g * repeats + n is repeat n
    of position g) followed by angio() on the card, ascans = height and depths = numdisplaypoints; the complex A-scans never reach
    the host.  The handle must have `averages` 1.  Returns what angio() returns.  Synchronous."""
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
    rec._check(rec.lib.fdoct_process_angio(rec.h, a.ctypes.data, capi._NP2DT[a.dtype], MEM_HOST, T, a.strides[1], C.byref(p), ptr("var"), ptr("decorr"),
                                           ptr("cdecorr"), ptr("power"), MEM_HOST))
    return _result(want, names, outs)


def process_angio_device(rec, d_frames_ptr, dtype, nframes, pitch_bytes, p, d_var_ptr, d_decorr_ptr, d_cdecorr_ptr, d_power_ptr):
    """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_process_angio(rec.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), C.byref(p), d_var_ptr, d_decorr_ptr,
                                           d_cdecorr_ptr, d_power_ptr, MEM_DEVICE))
