"""The binding of include/fdoct_vibro.h: phase-sensitive vibrometry from complex A-scans over time on the GPU -- a reference
surface's common-mode phase removed, the phase unwrapped over the frames, and per pixel the complex amplitude at up to 8 drive
frequencies, the RMS displacement, the net drift and the mean power.  The entry points live in libfdoct_vibro.so, a fifth add-on
library over libfdoct_hip.so; capi.load_library attaches them to the object it returns (attach, below).  Functions over a
Reconstructor, not methods of it.

    from fdoct_amd import vibrometry
    p = vibrometry.params(freq=[drive_hz / frame_rate_hz], ref=(surface_bin, 4), scale=lambda0 / (4 * np.pi * n_medium))
    out = vibrometry.process_vibro(rec, frames, p)     # out["amp"][0]: complex displacement amplitude, (height, depths)

ref is None, True (every depth) or (first, count), count 0 meaning up to the last depth.  A frequency is in cycles per frame,
in (0, 0.5].  A vibration a sin(2 pi nu t + psi) over a whole number of cycles gives amp = scale * (-1j) * a * exp(1j * psi)."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, FdoctError

# every symbol include/fdoct_vibro.h declares
VIBRO_ABI_SYMBOLS = ["fdoct_vibro_plan", "fdoct_vibro", "fdoct_process_vibro"]
WANTS = ("amp", "rms", "drift", "power")
RECT, HANN = 0, 1
MAX_FREQ = 8


class _CParams(C.Structure):
    """fdoct_vibro_params."""
    _fields_ = [("ref", C.c_int), ("ref_first", C.c_int), ("ref_count", C.c_int), ("detrend", C.c_int), ("window", C.c_int), ("nfreq", C.c_int),
                ("freq", C.c_double * MAX_FREQ), ("scale", C.c_double), ("min_power", C.c_double), ("chunk_steps", C.c_int)]


class _CInfo(C.Structure):
    """fdoct_vibro_info."""
    _fields_ = [("chunk_steps", C.c_int), ("chunks", C.c_int), ("workgroups", C.c_longlong), ("workspace_bytes", C.c_size_t)]


def library_path():
    """The add-on library of include/fdoct_vibro.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_vibro.so")


def attach(lib):
    """Loads libfdoct_vibro.so and attaches its entry points to the core library's object (capi.load_library calls this)."""
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % path)
    vib = C.CDLL(path)
    for name in VIBRO_ABI_SYMBOLS:
        setattr(lib, name, getattr(vib, name))
    lib.fdoct_vibro_plan.argtypes = [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(_CInfo)]
    lib.fdoct_vibro.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_CParams), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_vibro.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_CParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def params(freq=(), ref=None, detrend=0, window=RECT, scale=1.0, min_power=0.0, chunk_steps=0):
    """fdoct_vibro_params.  The library, not this function, refuses bad values -- except more than 8 frequencies, which do not fit
    the structure."""
    try:
        fr = [float(v) for v in freq]
        if ref is None or ref is False:
            use, first, count = 0, 0, 0
        else:
            use, (first, count) = 1, ((0, 0) if ref is True else ref)
        if len(fr) > MAX_FREQ:
            raise ValueError
        return _CParams(use, int(first), int(count), int(detrend), int(window), len(fr), (C.c_double * MAX_FREQ)(*fr), float(scale), float(min_power),
                        int(chunk_steps))
    except (TypeError, ValueError):
        raise FdoctError(-1, "freq holds at most 8 numbers, ref is None, True or (first, count)")


def _params(p):
    return p if isinstance(p, _CParams) else params(**p)


def plan(p, nframes, ascans, depths):
    """fdoct_vibro_plan: the geometry of a call as a dict (chunk_steps, chunks, workgroups, workspace_bytes), or FdoctError -1 where
    the call would be refused.  Needs no GPU."""
    p, info = _params(p), _CInfo()
    rc = capi.load_library().fdoct_vibro_plan(C.byref(p), int(nframes), int(ascans), int(depths), C.byref(info))
    if rc:
        raise FdoctError(rc, "fdoct_vibro_plan: 2..65536 frames, at most 2^24 pixels, at most 8 frequencies in (0, 0.5], a reference range "
                             "inside [0, depths), detrend and window 0 or 1, finite scale and min_power >= 0, chunk_steps >= 0")
    return {k: int(getattr(info, k)) for k, _ in _CInfo._fields_}


def _outputs(want, nfreq, ascans, depths):
    if isinstance(want, str):
        want = (want,)
    if want is None:
        want = WANTS if nfreq else WANTS[1:]
    if not want or any(w not in WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of %s, each once" % (WANTS,))
    shapes = {"amp": ((nfreq, ascans, depths), np.complex64), "rms": ((ascans, depths), np.float32), "drift": ((ascans, depths), np.float32),
              "power": ((ascans, depths), np.float32)}
    return tuple(want), {w: np.empty(*shapes[w]) for w in want}


def _result(want, names, outs):
    return outs[names[0]] if isinstance(want, str) else {w: outs[w] for w in names}


def vibro(rec, X, p, want=None):
    """fdoct_vibro on host memory: X is complex64 (nframes, ascans, depths), as process_complex returns it.  Returns a dict of the
    outputs `want` names (one name as a string: that output alone; None: all, without amp where there is no frequency): amp
    (nfreq, ascans, depths) complex64; rms, drift and power (ascans, depths) float32.  Synchronous."""
    a = np.asarray(X)
    if a.dtype != np.complex64 or a.ndim != 3 or a.size == 0:
        raise FdoctError(-1, "X must be complex64 of shape (nframes, ascans, depths)")
    a = np.ascontiguousarray(a)
    p = _params(p)
    T, H, D = a.shape
    plan(p, T, H, D)
    names, outs = _outputs(want, p.nfreq, H, D)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_vibro(rec.h, a.ctypes.data, MEM_HOST, T, H, D, C.byref(p), ptr("amp"), ptr("rms"), ptr("drift"), ptr("power"), MEM_HOST))
    return _result(want, names, outs)


def vibro_device(rec, d_re_im_ptr, nframes, ascans, depths, p, d_amp_ptr, d_rms_ptr, d_drift_ptr, d_power_ptr):
    """... on device-resident pairs into device memory (raw addresses; the pairs and d_amp_ptr aligned to 8 bytes, the others to 4;
    any output may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_vibro(rec.h, d_re_im_ptr, MEM_DEVICE, int(nframes), int(ascans), int(depths), C.byref(p), d_amp_ptr, d_rms_ptr,
                                   d_drift_ptr, d_power_ptr, MEM_DEVICE))


def process_vibro(rec, frames, p, want=None):
    """fdoct_process_vibro: process_complex's chain on `frames` (numpy, as process() takes them; time is the frame index) followed
    by vibro() on the card, ascans = height and depths = numdisplaypoints; the complex A-scans never reach the host.  The handle
    must have `averages` 1.  Returns what vibro() returns.  Synchronous."""
    a = np.ascontiguousarray(frames)
    if a.ndim == 2:
        a = a[None]
    if a.dtype not in capi._NP2DT:
        raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
    if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
        raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
    p = _params(p)
    T, H, D = a.shape[0], rec.cfg.height, rec.cfg.numdisplaypoints
    plan(p, T, H, D)
    names, outs = _outputs(want, p.nfreq, H, D)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_process_vibro(rec.h, a.ctypes.data, capi._NP2DT[a.dtype], MEM_HOST, T, a.strides[1], C.byref(p), ptr("amp"), ptr("rms"),
                                           ptr("drift"), ptr("power"), MEM_HOST))
    return _result(want, names, outs)


def process_vibro_device(rec, d_frames_ptr, dtype, nframes, pitch_bytes, p, d_amp_ptr, d_rms_ptr, d_drift_ptr, d_power_ptr):
    """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_process_vibro(rec.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), C.byref(p), d_amp_ptr, d_rms_ptr,
                                           d_drift_ptr, d_power_ptr, MEM_DEVICE))
