"""The binding of include/fdoct_ssada.h: split-spectrum amplitude decorrelation (SSADA) on the GPU -- the spectrum of every complex
A-scan split into Gaussian bands, every band transformed back, the repeats of a position reduced to angiography's amplitude
decorrelation band by band, and the bands averaged.  The entry points live in libfdoct_ssada.so, an eighth add-on library over
libfdoct_hip.so; capi.load_library attaches them to the object it returns (attach, below).  Functions over a Reconstructor, not
methods of it.

    from fdoct_amd import ssada
    p = ssada.params(repeats=4, bands=4, n=2048, win=(3, 5))
    out = ssada.process_ssada(rec, frames, p)     # out["decorr"]: (positions, height, depths), frames = positions * 4

The A-scans have the full transform length n (a handle with numdisplaypoints = numfftpoints).  Frame g * repeats + n is repeat n
of position g.  support = (k_first, k_count) is the range of spectral bins the bands share, count 0 meaning up to n; depth =
(first, count) the depths kept, count 0 meaning up to n // 2; win is (A-scans, depths), each 1 .. 16.  sigma is the bands'
Gaussian width in bins; None means half the band spacing, which needs n (or an explicit support count)."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, FdoctError

# every symbol include/fdoct_ssada.h declares
SSADA_ABI_SYMBOLS = ["fdoct_ssada_band_table", "fdoct_ssada_plan", "fdoct_ssada", "fdoct_process_ssada"]
WANTS = ("decorr", "band_decorr", "power", "bands")
MAX_WIN, MAX_REPEATS, MAX_BANDS = 16, 64, 16


class _CParams(C.Structure):
    """fdoct_ssada_params."""
    _fields_ = [("repeats", C.c_int), ("bands", C.c_int), ("sigma", C.c_double), ("k_first", C.c_int), ("k_count", C.c_int),
                ("depth_first", C.c_int), ("depth_count", C.c_int), ("win_ascans", C.c_int), ("win_depths", C.c_int),
                ("min_power", C.c_double), ("max_workspace_bytes", C.c_size_t)]


class _CInfo(C.Structure):
    """fdoct_ssada_info."""
    _fields_ = [("groups", C.c_int), ("depth_count", C.c_int), ("groups_per_pass", C.c_int), ("passes", C.c_int), ("lds_bytes", C.c_uint),
                ("workgroups", C.c_longlong), ("workspace_bytes", C.c_size_t)]


def library_path():
    """The add-on library of include/fdoct_ssada.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_ssada.so")


def attach(lib):
    """Loads libfdoct_ssada.so and attaches its entry points to the core library's object (capi.load_library calls this)."""
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % path)
    ssa = C.CDLL(path)
    for name in SSADA_ABI_SYMBOLS:
        setattr(lib, name, getattr(ssa, name))
    lib.fdoct_ssada_band_table.argtypes = [C.POINTER(_CParams), C.c_int, C.c_void_p]
    lib.fdoct_ssada_plan.argtypes = [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(_CInfo)]
    lib.fdoct_ssada.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_CParams), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_ssada.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_CParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def params(repeats=2, bands=4, sigma=None, support=(0, 0), depth=(0, 0), win=(1, 1), min_power=0.0, max_workspace_bytes=0, n=None):
    """fdoct_ssada_params.  sigma None: half the band spacing, (support count, or n - support first) / bands / 2.  The library, not
    this function, refuses bad values; what does not fit the structure is refused here."""
    try:
        (k0, kc), (d0, dc), (wa, wd) = support, depth, win
        if sigma is None:
            count = int(kc) if int(kc) else (int(n) - int(k0) if n is not None else None)
            if count is None:
                raise FdoctError(-1, "sigma=None needs n or a support with a count")
            sigma = 0.5 * count / int(bands)
        return _CParams(int(repeats), int(bands), float(sigma), int(k0), int(kc), int(d0), int(dc), int(wa), int(wd), float(min_power),
                        int(max_workspace_bytes))
    except (TypeError, ValueError, ZeroDivisionError):
        raise FdoctError(-1, "repeats and bands are numbers, support and depth are (first, count), win is (A-scans, depths)")


def _params(p, n=None):
    if isinstance(p, _CParams):
        return p
    kw = dict(p)
    kw.setdefault("n", n)
    return params(**kw)


def band_table(p, n):
    """fdoct_ssada_band_table: (bands, n) float32, G_m(q) evaluated in double and rounded.  Needs no GPU."""
    p, n = _params(p, n), int(n)
    out = np.empty((max(p.bands, 0), max(n, 0)), np.float32)
    rc = capi.load_library().fdoct_ssada_band_table(C.byref(p), n, out.ctypes.data)
    if rc:
        raise FdoctError(rc, "fdoct_ssada_band_table: n at least 1, bands 1..16, sigma finite and > 0, a support inside [0, n)")
    return out


def plan(p, nframes, ascans, n):
    """fdoct_ssada_plan: the geometry of a call as a dict (groups, depth_count, groups_per_pass, passes, lds_bytes, workgroups,
    workspace_bytes), or FdoctError where the call would be refused (-1 invalid, -2 unsupported).  Needs no GPU."""
    p, info = _params(p, n), _CInfo()
    rc = capi.load_library().fdoct_ssada_plan(C.byref(p), int(nframes), int(ascans), int(n), C.byref(info))
    if rc:
        raise FdoctError(rc, "fdoct_ssada_plan: n must be 2^a 3^b 5^c in 16..4096, repeats 2..64, bands 1..16, frames a positive multiple of "
                             "repeats with frames x bands at most 65536, at most 2^24 pixels kept, ranges inside [0, n) with a bin, sigma "
                             "finite and > 0, windows 1..16, finite min_power >= 0, a workspace cap that holds one group")
    return {k: int(getattr(info, k)) for k, _ in _CInfo._fields_}


def _outputs(want, groups, bands, repeats, ascans, dc):
    if isinstance(want, str):
        want = (want,)
    if want is None:
        want = WANTS
    if not want or any(w not in WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of %s, each once" % (WANTS,))
    shapes = {"decorr": ((groups, ascans, dc), np.float32), "power": ((groups, ascans, dc), np.float32),
              "band_decorr": ((groups, bands, ascans, dc), np.float32), "bands": ((groups, bands, repeats, ascans, dc), np.complex64)}
    return tuple(want), {w: np.empty(*shapes[w]) for w in want}


def _result(want, names, outs):
    return outs[names[0]] if isinstance(want, str) else {w: outs[w] for w in names}


def ssada(rec, X, p, want=None):
    """fdoct_ssada on host memory: X is complex64 (nframes, ascans, n), as process_complex returns it on a handle with
    numdisplaypoints = numfftpoints, nframes = groups * repeats.  Returns a dict of the outputs `want` names (one name as a string:
    that output alone; None: all four): decorr and power (groups, ascans, depths) float32, band_decorr (groups, bands, ascans,
    depths) float32, bands (groups, bands, repeats, ascans, depths) complex64.  Synchronous."""
    a = np.asarray(X)
    if a.dtype != np.complex64 or a.ndim != 3 or a.size == 0:
        raise FdoctError(-1, "X must be complex64 of shape (nframes, ascans, n)")
    a = np.ascontiguousarray(a)
    T, H, n = a.shape
    p = _params(p, n)
    info = plan(p, T, H, n)
    names, outs = _outputs(want, info["groups"], p.bands, p.repeats, H, info["depth_count"])
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_ssada(rec.h, a.ctypes.data, MEM_HOST, T, H, n, C.byref(p), ptr("decorr"), ptr("band_decorr"), ptr("power"), ptr("bands"),
                                   MEM_HOST))
    return _result(want, names, outs)


def ssada_device(rec, d_re_im_ptr, nframes, ascans, n, p, d_decorr_ptr, d_band_decorr_ptr, d_power_ptr, d_bands_ptr):
    """... on device-resident pairs into device memory (raw addresses; the pairs and d_bands_ptr aligned to 8 bytes, the other
    outputs to 4; any output may be None).  Enqueues on the handle's stream."""
    p = _params(p, n)
    rec._check(rec.lib.fdoct_ssada(rec.h, d_re_im_ptr, MEM_DEVICE, int(nframes), int(ascans), int(n), C.byref(p), d_decorr_ptr, d_band_decorr_ptr,
                                   d_power_ptr, d_bands_ptr, MEM_DEVICE))


def process_ssada(rec, frames, p, want=None):
    """fdoct_process_ssada: process_complex's chain on `frames` (numpy, as process() takes them; frame g * repeats + n is repeat n
    of position g) followed by ssada() on the card, ascans = height and n = numfftpoints; the complex A-scans never reach the host.
    The handle must have numdisplaypoints = numfftpoints and `averages` 1.  Returns what ssada() returns.  Synchronous."""
    a = np.ascontiguousarray(frames)
    if a.ndim == 2:
        a = a[None]
    if a.dtype not in capi._NP2DT:
        raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
    if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
        raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
    T, H, n = a.shape[0], rec.cfg.height, rec.cfg.numfftpoints
    if rec.cfg.numdisplaypoints != n:
        raise FdoctError(-2, "numdisplaypoints must equal numfftpoints: the bands are split from the full-length A-scan")
    p = _params(p, n)
    info = plan(p, T, H, n)
    names, outs = _outputs(want, info["groups"], p.bands, p.repeats, H, info["depth_count"])
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_process_ssada(rec.h, a.ctypes.data, capi._NP2DT[a.dtype], MEM_HOST, T, a.strides[1], C.byref(p), ptr("decorr"),
                                           ptr("band_decorr"), ptr("power"), ptr("bands"), MEM_HOST))
    return _result(want, names, outs)


def process_ssada_device(rec, d_frames_ptr, dtype, nframes, pitch_bytes, p, d_decorr_ptr, d_band_decorr_ptr, d_power_ptr, d_bands_ptr):
    """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
    p = _params(p, rec.cfg.numfftpoints)
    rec._check(rec.lib.fdoct_process_ssada(rec.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), C.byref(p), d_decorr_ptr,
                                           d_band_decorr_ptr, d_power_ptr, d_bands_ptr, MEM_DEVICE))
