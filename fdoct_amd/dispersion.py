"""The binding of include/fdoct_dispersion.h: a numerical dispersion search over a grid of (a2, a3) on the GPU, the source of the
table Reconstructor.set_dispersion_phase takes.  The entry points live in libfdoct_dispersion.so, a fourth add-on library over
libfdoct_hip.so; capi.load_library attaches them to the object it returns (attach, below).  Functions over a Reconstructor, not
methods of it.

A grid axis is (first, step, count): a2 = (-24.0, 4.0, 13) holds -24, -20, ..., 24.  depth = (first, count) is the range of bins
the sums run over; count 0 means up to n // 2.  Candidate c = i2 * a3_count + i3.

The calibration recipe: a handle with the instrument's configuration and numdisplaypoints = numfftpoints,
process_search on a few frames of a sample with sharp reflectors, then set_dispersion_phase(result["cos_sin"]) on the instrument's
own handle."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, FdoctError

# every symbol include/fdoct_dispersion.h declares
DISPERSION_ABI_SYMBOLS = ["fdoct_dispersion_phase_table", "fdoct_dispersion_plan", "fdoct_dispersion_search",
                          "fdoct_process_dispersion_search"]
WANTS = ("sums", "row_sums", "best", "cos_sin")


class _CGrid(C.Structure):
    """fdoct_dispersion_grid."""
    _fields_ = [("a2_first", C.c_double), ("a2_step", C.c_double), ("a2_count", C.c_int), ("a3_first", C.c_double), ("a3_step", C.c_double),
                ("a3_count", C.c_int), ("depth_first", C.c_int), ("depth_count", C.c_int)]


class _CBest(C.Structure):
    """fdoct_dispersion_best."""
    _fields_ = [("index", C.c_int), ("i2", C.c_int), ("i3", C.c_int), ("a2", C.c_double), ("a3", C.c_double), ("metric", C.c_double)]


class _CInfo(C.Structure):
    """fdoct_dispersion_info."""
    _fields_ = [("candidates", C.c_int), ("per_workgroup", C.c_int), ("chunks", C.c_int), ("lds_bytes", C.c_uint), ("workgroups", C.c_longlong),
                ("workspace_bytes", C.c_size_t)]


BEST_DTYPE = np.dtype([("index", np.int32), ("i2", np.int32), ("i3", np.int32), ("pad", np.int32), ("a2", np.float64), ("a3", np.float64),
                       ("metric", np.float64)])   # fdoct_dispersion_best as a numpy record: what a device buffer of it reads as


def library_path():
    """The add-on library of include/fdoct_dispersion.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_dispersion.so")


def attach(lib):
    """Loads libfdoct_dispersion.so and attaches its entry points to the core library's object (capi.load_library calls this)."""
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % path)
    disp = C.CDLL(path)
    for name in DISPERSION_ABI_SYMBOLS:
        setattr(lib, name, getattr(disp, name))
    lib.fdoct_dispersion_phase_table.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p]
    lib.fdoct_dispersion_plan.argtypes = [C.POINTER(_CGrid), C.c_int, C.c_int, C.POINTER(_CInfo)]
    lib.fdoct_dispersion_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_CGrid), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_dispersion_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_CGrid),
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def grid(a2, a3, depth=(0, 0)):
    """fdoct_dispersion_grid from (first, step, count), (first, step, count) and (depth_first, depth_count)."""
    try:
        (f2, s2, c2), (f3, s3, c3), (d0, dc) = a2, a3, depth
        return _CGrid(float(f2), float(s2), int(c2), float(f3), float(s3), int(c3), int(d0), int(dc))
    except (TypeError, ValueError):
        raise FdoctError(-1, "a2 and a3 are (first, step, count), depth is (first, count)")


def candidate(a2, a3, c):
    """(a2, a3) of candidate index c, as the library evaluates them: first + i * step in double."""
    i2, i3 = divmod(int(c), int(a3[2]))
    return float(a2[0]) + i2 * float(a2[1]), float(a3[0]) + i3 * float(a3[1])


def phase_table(n, a2, a3):
    """fdoct_dispersion_phase_table: (n, 2) float32 (cos, sin) of phi(q) = a2 x^2 + a3 x^3, x = (q - n/2) / (n/2).  Needs no GPU."""
    n = int(n)
    out = np.empty((max(n, 0), 2), np.float32)
    rc = capi.load_library().fdoct_dispersion_phase_table(n, float(a2), float(a3), out.ctypes.data)
    if rc:
        raise FdoctError(rc, "fdoct_dispersion_phase_table: n must be at least 1, a2 and a3 finite")
    return out


def plan(a2, a3, rows, n, depth=(0, 0)):
    """fdoct_dispersion_plan: the geometry of a call as a dict (candidates, per_workgroup, chunks, lds_bytes, workgroups,
    workspace_bytes), or FdoctError where the call would be refused (-1 invalid, -2 unsupported).  Needs no GPU."""
    g, info = grid(a2, a3, depth), _CInfo()
    rc = capi.load_library().fdoct_dispersion_plan(C.byref(g), int(rows), int(n), C.byref(info))
    if rc:
        raise FdoctError(rc, "fdoct_dispersion_plan: n must be 2^a 3^b 5^c in 16..4096, 1..65536 candidates, rows x candidates at most "
                             "2^24, finite firsts and steps, a depth range inside [0, n) with a bin")
    return {k: int(getattr(info, k)) for k, _ in _CInfo._fields_}


def _outputs(want, rows, K, n):
    if isinstance(want, str):
        want = (want,)
    if not want or any(w not in WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of %s, each once" % (WANTS,))
    shapes = {"sums": ((K, 2), np.float64), "row_sums": ((rows, K, 2), np.float64), "best": ((1,), BEST_DTYPE), "cos_sin": ((n, 2), np.float32)}
    return tuple(want), {w: np.empty(*shapes[w]) for w in want}


def _result(want, names, outs):
    if "best" in outs:
        b = outs["best"][0]
        outs["best"] = {k: (int(b[k]) if k in ("index", "i2", "i3") else float(b[k])) for k in ("index", "i2", "i3", "a2", "a3", "metric")}
    return outs[names[0]] if isinstance(want, str) else {w: outs[w] for w in names}


def search(rec, X, a2, a3, depth=(0, 0), want=WANTS):
    """fdoct_dispersion_search on host memory: X is complex64 (..., n), every leading axis a row, as process_complex returns it on a
    handle with numdisplaypoints = numfftpoints.  Returns a dict of the outputs `want` names (one name as a string: that output
    alone): sums (K, 2) and row_sums (rows, K, 2) float64 (S2, S4); best a dict (index, i2, i3, a2, a3, metric); cos_sin (n, 2)
    float32, what set_dispersion_phase takes.  Synchronous."""
    a = np.asarray(X)
    if a.dtype != np.complex64 or a.ndim < 1 or a.size == 0:
        raise FdoctError(-1, "X must be complex64 of shape (..., n)")
    a = np.ascontiguousarray(a).reshape(-1, a.shape[-1])
    rows, n = a.shape
    g = grid(a2, a3, depth)
    K = plan(a2, a3, rows, n, depth)["candidates"]
    names, outs = _outputs(want, rows, K, n)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_dispersion_search(rec.h, a.ctypes.data, MEM_HOST, rows, n, C.byref(g), ptr("sums"), ptr("row_sums"), ptr("best"),
                                               ptr("cos_sin"), MEM_HOST))
    return _result(want, names, outs)


def search_device(rec, d_re_im_ptr, rows, n, a2, a3, d_sums_ptr, d_row_sums_ptr, d_best_ptr, d_cos_sin_ptr, depth=(0, 0)):
    """... on device-resident pairs into device memory (raw addresses, each aligned to 8 bytes; any output may be None; d_best_ptr
    holds one fdoct_dispersion_best, BEST_DTYPE).  Enqueues on the handle's stream."""
    g = grid(a2, a3, depth)
    rec._check(rec.lib.fdoct_dispersion_search(rec.h, d_re_im_ptr, MEM_DEVICE, int(rows), int(n), C.byref(g), d_sums_ptr, d_row_sums_ptr, d_best_ptr,
                                               d_cos_sin_ptr, MEM_DEVICE))


def process_search(rec, frames, a2, a3, depth=(0, 0), want=WANTS):
    """fdoct_process_dispersion_search: process_complex's chain on `frames` (numpy, as process() takes them) followed by search() on
    the card, rows = nframes x height; the complex A-scans never reach the host.  The handle must have numdisplaypoints =
    numfftpoints and `averages` 1.  If it has a phase set, the result is the residual on top of it.  Returns what search() returns.
    Synchronous."""
    a = np.ascontiguousarray(frames)
    if a.ndim == 2:
        a = a[None]
    if a.dtype not in capi._NP2DT:
        raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
    if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
        raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
    nframes, rows, n = a.shape[0], a.shape[0] * rec.cfg.height, rec.cfg.numfftpoints
    if rec.cfg.numdisplaypoints != n:
        raise FdoctError(-2, "numdisplaypoints must equal numfftpoints: a calibration handle shows the full length")
    g = grid(a2, a3, depth)
    K = plan(a2, a3, rows, n, depth)["candidates"]
    names, outs = _outputs(want, rows, K, n)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_process_dispersion_search(rec.h, a.ctypes.data, capi._NP2DT[a.dtype], MEM_HOST, nframes, a.strides[1], C.byref(g),
                                                       ptr("sums"), ptr("row_sums"), ptr("best"), ptr("cos_sin"), MEM_HOST))
    return _result(want, names, outs)


def process_search_device(rec, d_frames_ptr, dtype, nframes, pitch_bytes, a2, a3, d_sums_ptr, d_row_sums_ptr, d_best_ptr, d_cos_sin_ptr,
                          depth=(0, 0)):
    """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
    g = grid(a2, a3, depth)
    rec._check(rec.lib.fdoct_process_dispersion_search(rec.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), C.byref(g),
                                                       d_sums_ptr, d_row_sums_ptr, d_best_ptr, d_cos_sin_ptr, MEM_DEVICE))
