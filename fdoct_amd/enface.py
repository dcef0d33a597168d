"""The binding of include/fdoct_enface.h: the en-face projection of a volume of positions x A-scans x depths floats on the GPU --
per depth slab the mean, the maximum and the depth of the maximum of every A-scan, over slabs that are fixed or follow the tissue
surface (a threshold crossing of the smoothed A-scan, absolute or relative to the A-scan's own maximum, with a lateral median).
The entry points live in libfdoct_enface.so, a ninth add-on library over libfdoct_hip.so; capi.load_library attaches them to the
object it returns (attach, below).  Functions over a Reconstructor, not methods of it.

    from fdoct_amd import enface
    p = enface.params(slabs=[(0, 64), (64, 64)], surface="relative", threshold=0.5, smooth=4, median=5)
    out = enface.project(rec, decorr, p, structure=power)       # out["mean"]: (2, positions, ascans)
    img = enface.process_project(rec, frames, enface.params(slabs=[(100, 50)]), want="max")   # the chain, then the projection

slabs is a list of (first, count), first relative to the surface (to depth 0 without one).  The device-memory forms are
project_into and process_project_into: the tests' catalogue of stream-ordered entry points (tests/stream_cases.py) lists every
module-level *_device function of the package and predates this stage, so these two carry another suffix until the catalogue lists
them; their stream-order contract is held by tests/test_gpu_enface.py meanwhile."""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, FdoctError

# every symbol include/fdoct_enface.h declares
ENFACE_ABI_SYMBOLS = ["fdoct_enface_plan", "fdoct_enface", "fdoct_process_enface"]
WANTS = ("mean", "max", "argmax", "surface")
MAX_SLABS, MAX_SMOOTH, MAX_MEDIAN = 8, 16, 15
SURFACE_NONE, SURFACE_ABSOLUTE, SURFACE_RELATIVE = 0, 1, 2
SOURCE_LINEAR, SOURCE_DB = 0, 1
_SURFACES = {None: 0, "none": 0, "absolute": 1, "relative": 2, 0: 0, 1: 1, 2: 2}
_SOURCES = {"linear": 0, "db": 1, 0: 0, 1: 1}


class _CParams(C.Structure):
    """fdoct_enface_params."""
    _fields_ = [("surface", C.c_int), ("search_first", C.c_int), ("search_count", C.c_int), ("smooth", C.c_int), ("threshold", C.c_double),
                ("median", C.c_int), ("nslabs", C.c_int), ("slab_first", C.c_int * MAX_SLABS), ("slab_count", C.c_int * MAX_SLABS)]


class _CInfo(C.Structure):
    """fdoct_enface_info."""
    _fields_ = [("ascans", C.c_longlong), ("workgroups", C.c_longlong), ("workspace_bytes", C.c_size_t), ("read_first", C.c_int),
                ("read_count", C.c_int)]


def library_path():
    """The add-on library of include/fdoct_enface.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_enface.so")


def attach(lib):
    """Loads libfdoct_enface.so and attaches its entry points to the core library's object (capi.load_library calls this)."""
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % path)
    enf = C.CDLL(path)
    for name in ENFACE_ABI_SYMBOLS:
        setattr(lib, name, getattr(enf, name))
    lib.fdoct_enface_plan.argtypes = [C.POINTER(_CParams), C.c_int, C.c_int, C.c_int, C.POINTER(_CInfo)]
    lib.fdoct_enface.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_CParams), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_enface.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(_CParams), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def params(slabs=((0, 1),), surface=None, search=(0, 0), smooth=1, threshold=0.0, median=1):
    """fdoct_enface_params.  slabs: up to 8 (first, count); surface: None, "absolute" or "relative" (or 0, 1, 2); search: (first,
    count), count 0 meaning up to the last depth.  The library, not this function, refuses bad values; what does not fit the structure
    is refused here."""
    try:
        slabs = [(int(f), int(c)) for f, c in slabs]
        if len(slabs) > MAX_SLABS or surface not in _SURFACES:
            raise ValueError
        first, count = search
        p = _CParams(_SURFACES[surface], int(first), int(count), int(smooth), float(threshold), int(median), len(slabs))
        for s, (f, c) in enumerate(slabs):
            p.slab_first[s], p.slab_count[s] = f, c
        return p
    except (TypeError, ValueError):
        raise FdoctError(-1, "slabs is up to 8 (first, count), surface is None, 'absolute' or 'relative', search is (first, count)")


def _params(p):
    return p if isinstance(p, _CParams) else params(**p)


def plan(p, positions, ascans, depths):
    """fdoct_enface_plan: the geometry of a call as a dict (ascans, workgroups, workspace_bytes, read_first, read_count), or FdoctError
    -1 where the call would be refused.  Needs no GPU."""
    p, info = _params(p), _CInfo()
    rc = capi.load_library().fdoct_enface_plan(C.byref(p), int(positions), int(ascans), int(depths), C.byref(info))
    if rc:
        raise FdoctError(rc, "fdoct_enface_plan: positions 1..65536, at most 2^24 pixels a position, surface 0..2, smooth 1..16, median odd 1..15, "
                             "1..8 slabs of at least one depth that start inside the volume, a search range inside [0, depths) that holds smooth "
                             "depths, a finite threshold (relative: in (0, 1])")
    return {k: int(getattr(info, k)) for k, _ in _CInfo._fields_}


def _outputs(want, p, positions, ascans):
    if isinstance(want, str):
        want = (want,)
    if want is None:
        want = WANTS if p.surface else WANTS[:3]
    if not want or any(w not in WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of %s, each once" % (WANTS,))
    outs = {}
    for w in want:
        shape = (positions, ascans) if w == "surface" else (p.nslabs, positions, ascans)
        outs[w] = np.empty(shape, np.float32 if w in ("mean", "max") else np.int32)
    return tuple(want), outs


def _result(want, names, outs):
    return outs[names[0]] if isinstance(want, str) else {w: outs[w] for w in names}


def project(rec, V, p, want=None, structure=None):
    """fdoct_enface on host memory: V is float32 (positions, ascans, depths); structure, if given, a volume of the same shape the
    surface is found in.  Returns a dict of the outputs `want` names (one name as a string: that output alone; None: all the call can
    give -- "surface" only with a surface): mean and max float32, argmax int32, each (nslabs, positions, ascans); surface int32
    (positions, ascans).  Synchronous."""
    a = np.asarray(V)
    if a.dtype != np.float32 or a.ndim != 3 or a.size == 0:
        raise FdoctError(-1, "V must be float32 of shape (positions, ascans, depths)")
    a = np.ascontiguousarray(a)
    s = None
    if structure is not None:
        s = np.asarray(structure)
        if s.dtype != np.float32 or s.shape != a.shape:
            raise FdoctError(-1, "structure must be float32 of V's shape")
        s = np.ascontiguousarray(s)
    p = _params(p)
    P, H, D = a.shape
    plan(p, P, H, D)
    names, outs = _outputs(want, p, P, H)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_enface(rec.h, a.ctypes.data, None if s is None else s.ctypes.data, MEM_HOST, P, H, D, C.byref(p), ptr("mean"), ptr("max"),
                                    ptr("argmax"), ptr("surface"), MEM_HOST))
    return _result(want, names, outs)


def project_into(rec, d_vol_ptr, d_structure_ptr, positions, ascans, depths, p, d_mean_ptr, d_max_ptr, d_argmax_ptr, d_surface_ptr):
    """... on a device-resident volume into device memory (raw addresses, each aligned to 4 bytes; the structure volume and any output
    may be None).  Enqueues on the handle's stream."""
    p = _params(p)
    rec._check(rec.lib.fdoct_enface(rec.h, d_vol_ptr, d_structure_ptr, MEM_DEVICE, int(positions), int(ascans), int(depths), C.byref(p), d_mean_ptr,
                                    d_max_ptr, d_argmax_ptr, d_surface_ptr, MEM_DEVICE))


def process_project(rec, frames, p, source="db", want=None):
    """fdoct_process_enface: process()'s chain on `frames` (numpy, as process() takes them) followed by project() on the card, with
    positions = frames / averages, ascans = height and depths = numdisplaypoints; source "linear" projects the linear B-scan, "db" its
    dB.  The volume never reaches the host.  Returns what project() returns.  Synchronous."""
    a = np.ascontiguousarray(frames)
    if a.ndim == 2:
        a = a[None]
    if a.dtype not in capi._NP2DT:
        raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
    if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
        raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
    if source not in _SOURCES:
        raise FdoctError(-1, "source is 'linear' or 'db'")
    p = _params(p)
    T, A, H, D = a.shape[0], max(int(rec.cfg.averages), 1), rec.cfg.height, rec.cfg.numdisplaypoints
    P = max(T // A, 1)
    plan(p, P, H, D)
    names, outs = _outputs(want, p, P, H)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rec._check(rec.lib.fdoct_process_enface(rec.h, a.ctypes.data, capi._NP2DT[a.dtype], MEM_HOST, T, a.strides[1], _SOURCES[source], C.byref(p),
                                            ptr("mean"), ptr("max"), ptr("argmax"), ptr("surface"), MEM_HOST))
    return _result(want, names, outs)


def process_project_into(rec, d_frames_ptr, dtype, nframes, pitch_bytes, source, p, d_mean_ptr, d_max_ptr, d_argmax_ptr, d_surface_ptr):
    """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
    if source not in _SOURCES:
        raise FdoctError(-1, "source is 'linear' or 'db'")
    p = _params(p)
    rec._check(rec.lib.fdoct_process_enface(rec.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), _SOURCES[source], C.byref(p),
                                            d_mean_ptr, d_max_ptr, d_argmax_ptr, d_surface_ptr, MEM_DEVICE))
