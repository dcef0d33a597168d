"""ctypes binding of include/fdoct.h (libfdoct_hip.so) and the host-side mirror
of the reference's processing block.

The reference (hn-88/FDOCT) has no operator/plugin API: the block is inlined in
``main()`` (BscanFFT.cpp:1123-1240) and configured by the ini values read at
BscanFFT.cpp:395-484.  ``Config`` therefore carries exactly those names
(``numfftpoints``, ``numdisplaypoints``, ``averages``, ``lambdamin`` ...) and
``Reconstructor`` exposes the state the key handlers capture
(``set_background`` = the 'b' key, main:1000-1075; ``set_pi_frame`` = 'p',
main:1077-1099) plus ``process`` = one pass of main:1123-1240 over a batch.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

DTYPE_U8, DTYPE_U16, DTYPE_F32, DTYPE_F64 = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED = 0, 1
VARIANT_MAIN, VARIANT_SIM = 0, 1

_NP2DT = {np.dtype(np.uint8): DTYPE_U8, np.dtype(np.uint16): DTYPE_U16, np.dtype(np.float32): DTYPE_F32,
          np.dtype(np.float64): DTYPE_F64}


class FdoctError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fdoct error %d: %s" % (code, msg))
        self.code = code


class _CConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("numfftpoints", C.c_int32), ("numdisplaypoints", C.c_int32),
                ("increasefftpointsmultiplier", C.c_int32), ("averages", C.c_int32),
                ("rowwisenormalize", C.c_int32), ("donotnormalize", C.c_int32), ("movavgn", C.c_int32),
                ("variant", C.c_int32), ("dc_mask", C.c_int32), ("device", C.c_int32),
                ("lambdamin", C.c_double), ("lambdamax", C.c_double)]


class _CTiming(C.Structure):
    _fields_ = [("last_process_ms", C.c_double), ("last_kernel_ms", C.c_double),
                ("resample_stage_ms", C.c_double), ("fft_stage_ms", C.c_double), ("ascans", C.c_uint64),
                ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64)]


@dataclass
class Config:
    """The ini values / locals the block reads (BscanFFT.cpp:395-484, 544-545)."""
    width: int
    height: int
    numfftpoints: int
    numdisplaypoints: int
    increasefftpointsmultiplier: int = 1
    averages: int = 1
    rowwisenormalize: int = 0
    donotnormalize: int = 1
    movavgn: int = 0
    variant: int = VARIANT_MAIN
    dc_mask: int = 1
    device: int = 0
    lambdamin: float = 816e-9
    lambdamax: float = 884e-9


def library_path():
    """The in-tree HIP library.  FDOCT_LIB names another build of the SAME product library (tuning variants from
    tools/mkvariant.sh, A/B runs): never a different implementation, and never anything under oracle/."""
    override = os.environ.get("FDOCT_LIB")
    if override:
        return os.path.abspath(override)
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_hip.so")


_lib = None

# every symbol include/fdoct.h declares
ABI_SYMBOLS = [
    "fdoct_version", "fdoct_create", "fdoct_destroy", "fdoct_last_error", "fdoct_set_stream",
    "fdoct_set_background", "fdoct_set_pi_frame", "fdoct_set_dark", "fdoct_set_window",
    "fdoct_set_resample_table", "fdoct_set_lambda_range", "fdoct_set_dispersion_phase",
    "fdoct_build_resample_table", "fdoct_build_window", "fdoct_build_colormap_jet", "fdoct_get_resample_table", "fdoct_get_window",
    "fdoct_process", "fdoct_process_async", "fdoct_synchronize", "fdoct_get_timing", "fdoct_set_launch",
    "fdoct_export_state", "fdoct_import_state", "fdoct_set_plan", "fdoct_set_staged", "fdoct_get_ylin", "fdoct_clone_to_device", "fdoct_device_count", "fdoct_shard_frames",
    "fdoct_set_frontend", "fdoct_frontend",
    "fdoct_set_timing", "fdoct_set_averages", "fdoct_set_bandpass", "fdoct_host_alloc", "fdoct_host_free", "fdoct_set_host_staging", "fdoct_get_host_staging", "fdoct_display", "fdoct_set_colormap", "fdoct_get_colormap", "fdoct_lockin_db",
    "fdoct_last_kernel", "fdoct_set_jit", "fdoct_jit_note", "fdoct_jit_compile_check", "fdoct_set_precise_division", "fdoct_prepare", "fdoct_broadcast_state_rccl",
]

# every symbol include/fdoct_roi.h declares: the B-scan readouts (a header and translation unit of their own, so that the ABI
# of include/fdoct.h above stays as it is)
ROI_ABI_SYMBOLS = [
    "fdoct_ascan_minmax", "fdoct_roi_mean", "fdoct_set_peakhold_roi", "fdoct_peakhold", "fdoct_get_peakhold",
    "fdoct_clear_peakhold", "fdoct_vibration_profile", "fdoct_besseldb_inverse",
]

# every symbol include/fdoct_capture.h declares: the reference frames captured from camera frames, likewise on their own
CAPTURE_ABI_SYMBOLS = ["fdoct_capture_reference", "fdoct_get_reference", "fdoct_frame_minmax", "fdoct_normalize_minmax"]
# every symbol include/fdoct_lowpass.h declares: BscanDark's lpfilter and the capture's two options, likewise on their own
LOWPASS_ABI_SYMBOLS = ["fdoct_set_capture_options", "fdoct_get_capture_options", "fdoct_lowpass_rows"]
# every symbol include/fdoct_bscanbin.h declares: spinjnt's output binning between the linear B-scan and its dB, likewise on its own
BSCANBIN_ABI_SYMBOLS = ["fdoct_bscanbin_size", "fdoct_bscanbin_taps", "fdoct_bscan_bin"]
# every symbol include/fdoct_colour.h declares: the webcam's interleaved B,G,R frames (channelnum), likewise on their own
COLOUR_ABI_SYMBOLS = ["fdoct_set_colour_input", "fdoct_get_colour_input", "fdoct_colour_extract", "fdoct_colour_sum_scale"]
# every symbol include/fdoct_manualavg.h declares: manual averaging of B-scans (manualaveraging / manualaverages), likewise on its own
MANUALAVG_ABI_SYMBOLS = ["fdoct_manualavg_plan", "fdoct_manualavg_begin", "fdoct_manualavg_add", "fdoct_manualavg_state",
                         "fdoct_manualavg_end"]
# every symbol include/fdoct_saveframes.h declares: per-frame saves while averaging (saveframes) and the chain's raw-magnitudes
# switch, likewise on their own
SAVEFRAMES_ABI_SYMBOLS = ["fdoct_set_raw_magnitudes", "fdoct_get_raw_magnitudes", "fdoct_saveframes"]
# every symbol include/fdoct_calibrate.h declares: BscanDark's calibration on the device (normalisations, held captures,
# composition).  They live in libfdoct_calibrate.so, an add-on library over libfdoct_hip.so (whose exported symbols are a closed
# set); load_library attaches them to the object it returns
CALIBRATE_ABI_SYMBOLS = ["fdoct_normalize_rows_minmax", "fdoct_calibrate_capture", "fdoct_calibrate_compose", "fdoct_calibrate_state",
                         "fdoct_calibrate_clear"]
# every symbol include/fdoct_complex.h declares: the complex A-scan (re, im) of the chain.  It lives in libfdoct_complex.so, a second
# add-on library over libfdoct_hip.so; load_library attaches it likewise
COMPLEX_ABI_SYMBOLS = ["fdoct_process_complex"]
# every symbol include/fdoct_doppler.h declares: phase-resolved Doppler from complex A-scans.  They live in libfdoct_doppler.so, a
# third add-on library over libfdoct_hip.so; load_library attaches them likewise
DOPPLER_ABI_SYMBOLS = ["fdoct_doppler_size", "fdoct_doppler", "fdoct_process_doppler"]
# fdoct_doppler_axis (include/fdoct_doppler.h)
DOPPLER_ASCANS, DOPPLER_FRAMES = 0, 1
# fdoct_cal_slot (include/fdoct_calibrate.h)
CAL_DARK, CAL_REFERENCE, CAL_SAMPLE = range(3)
# fdoct_manualavg_mode (include/fdoct_manualavg.h)
MANUALAVG_REFERENCE, MANUALAVG_KEEP_ALL = 0, 1
# fdoct_ref_role (include/fdoct_capture.h)
REF_BACKGROUND, REF_PI, REF_DARK, REF_NONE = range(4)

# fdoct_kernel (include/fdoct.h): what fdoct_last_kernel returns
KERNEL_NONE, KERNEL_FUSED, KERNEL_FUSED_TRANSPOSED, KERNEL_FUSED_STAGED, KERNEL_WAVE, KERNEL_WAVE_JIT, KERNEL_GENERIC, KERNEL_LONG_ROWS = range(8)


def jit_compile_check(width, multiplier, numfftpoints, numdisplaypoints, dtype=None, gcn_arch="gfx950"):
    """fdoct_jit_compile_check: (code object bytes or -1, reason).  Needs no GPU."""
    buf = C.create_string_buffer(1024)
    n = load_library().fdoct_jit_compile_check(width, multiplier, numfftpoints, numdisplaypoints, DTYPE_U16 if dtype is None else dtype,
                                               gcn_arch.encode(), buf, len(buf))
    return int(n), buf.value.decode()


def shard_frames(nframes_total, averages, part, nparts):
    """fdoct_shard_frames: [start, stop) frames of part `part` (the rule fdoct_amd/dist.py::shard_frames states in Python)."""
    first, count = C.c_int(), C.c_int()
    rc = load_library().fdoct_shard_frames(nframes_total, averages, part, nparts, C.byref(first), C.byref(count))
    if rc:
        raise FdoctError(rc, "fdoct_shard_frames: bad arguments")
    return first.value, first.value + count.value


def calibrate_library_path():
    """The add-on library of include/fdoct_calibrate.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_calibrate.so")


def complex_library_path():
    """The add-on library of include/fdoct_complex.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_complex.so")


def doppler_library_path():
    """The add-on library of include/fdoct_doppler.h, in the package next to the in-tree core library it is linked against."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdoct_doppler.so")


class _CDopplerParams(C.Structure):
    """fdoct_doppler_params (include/fdoct_doppler.h)."""
    _fields_ = [("axis", C.c_int), ("lag", C.c_int), ("win_ascans", C.c_int), ("win_depths", C.c_int), ("bulk", C.c_int),
                ("bulk_first", C.c_int), ("bulk_count", C.c_int), ("scale", C.c_double), ("min_power", C.c_double)]


def load_library():
    """Loads the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1; the first copy of a
    # soname loaded into the process is the one everybody gets.  If torch is going to share this
    # process (tests, bench.py: device tensors and streams come from it), let its copy load first --
    # the other order leaves torch without a visible GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` "
                             "(or __graft_entry__.build()); there is no CPU fallback" % path)
    lib = C.CDLL(path)
    lib.fdoct_version.restype = C.c_char_p
    lib.fdoct_last_error.restype = C.c_char_p
    lib.fdoct_last_error.argtypes = [C.c_void_p]
    lib.fdoct_create.argtypes = [C.POINTER(_CConfig), C.POINTER(C.c_void_p)]
    lib.fdoct_destroy.argtypes = [C.c_void_p]
    lib.fdoct_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    for name in ("fdoct_set_background", "fdoct_set_pi_frame", "fdoct_set_dark"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t]
    lib.fdoct_set_window.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_set_resample_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_set_lambda_range.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.fdoct_set_dispersion_phase.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_build_resample_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                               C.c_void_p]
    lib.fdoct_build_window.argtypes = [C.c_int, C.c_void_p]
    lib.fdoct_build_colormap_jet.argtypes = [C.c_void_p]
    lib.fdoct_get_resample_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_get_window.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int]
    lib.fdoct_process_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_int]
    lib.fdoct_synchronize.argtypes = [C.c_void_p]
    lib.fdoct_get_timing.argtypes = [C.c_void_p, C.POINTER(_CTiming)]
    lib.fdoct_set_launch.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fdoct_set_plan.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fdoct_set_staged.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_get_ylin.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.fdoct_clone_to_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.fdoct_shard_frames.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fdoct_set_timing.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_set_bandpass.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_set_averages.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_host_alloc.argtypes = [C.c_size_t]
    lib.fdoct_host_alloc.restype = C.c_void_p
    lib.fdoct_host_free.argtypes = [C.c_void_p]
    lib.fdoct_host_free.restype = None
    lib.fdoct_set_host_staging.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_get_host_staging.argtypes = [C.c_void_p]
    lib.fdoct_set_frontend.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.fdoct_frontend.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p]
    lib.fdoct_display.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_set_colormap.argtypes = [C.c_void_p, C.c_void_p]
    lib.fdoct_get_colormap.argtypes = [C.c_void_p, C.c_void_p]
    lib.fdoct_lockin_db.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    lib.fdoct_last_kernel.argtypes = [C.c_void_p]
    lib.fdoct_set_jit.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_set_precise_division.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_prepare.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fdoct_broadcast_state_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_jit_note.argtypes = [C.c_void_p]
    lib.fdoct_jit_note.restype = C.c_char_p
    lib.fdoct_jit_compile_check.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    lib.fdoct_jit_compile_check.restype = C.c_longlong
    lib.fdoct_export_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.fdoct_import_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    # include/fdoct_roi.h
    lib.fdoct_ascan_minmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_roi_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p, C.c_int]
    lib.fdoct_set_peakhold_roi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.fdoct_peakhold.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.fdoct_get_peakhold.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fdoct_clear_peakhold.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_vibration_profile.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fdoct_besseldb_inverse.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    # include/fdoct_capture.h
    lib.fdoct_capture_reference.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    lib.fdoct_get_reference.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    lib.fdoct_frame_minmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_int]
    lib.fdoct_normalize_minmax.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double]
    # include/fdoct_lowpass.h
    lib.fdoct_set_capture_options.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fdoct_get_capture_options.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fdoct_lowpass_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int]
    # include/fdoct_bscanbin.h
    lib.fdoct_bscanbin_size.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fdoct_bscanbin_taps.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.fdoct_bscan_bin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
    # include/fdoct_colour.h
    lib.fdoct_set_colour_input.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_get_colour_input.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.fdoct_colour_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.fdoct_colour_sum_scale.argtypes = []
    lib.fdoct_colour_sum_scale.restype = C.c_double
    # include/fdoct_manualavg.h
    lib.fdoct_manualavg_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fdoct_manualavg_begin.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int]
    lib.fdoct_manualavg_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.POINTER(C.c_int)]
    lib.fdoct_manualavg_state.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.c_void_p]
    lib.fdoct_manualavg_end.argtypes = [C.c_void_p]
    # include/fdoct_saveframes.h
    lib.fdoct_set_raw_magnitudes.argtypes = [C.c_void_p, C.c_int]
    lib.fdoct_get_raw_magnitudes.argtypes = [C.c_void_p]
    lib.fdoct_saveframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    # include/fdoct_calibrate.h: the add-on library's entry points, attached to the core library's object
    cal_path = calibrate_library_path()
    if not os.path.exists(cal_path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % cal_path)
    cal = C.CDLL(cal_path)
    for name in CALIBRATE_ABI_SYMBOLS:
        setattr(lib, name, getattr(cal, name))
    lib.fdoct_normalize_rows_minmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_double, C.c_double,
                                                C.c_int, C.c_void_p, C.c_int]
    lib.fdoct_calibrate_capture.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    lib.fdoct_calibrate_compose.argtypes = [C.c_void_p, C.c_void_p]
    lib.fdoct_calibrate_state.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.fdoct_calibrate_clear.argtypes = [C.c_void_p]
    # include/fdoct_complex.h: likewise
    cx_path = complex_library_path()
    if not os.path.exists(cx_path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % cx_path)
    cx = C.CDLL(cx_path)
    for name in COMPLEX_ABI_SYMBOLS:
        setattr(lib, name, getattr(cx, name))
    lib.fdoct_process_complex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    # include/fdoct_doppler.h: likewise
    dop_path = doppler_library_path()
    if not os.path.exists(dop_path):
        raise FdoctError(-3, "%s not found: build it with `make -C fdoct_amd/csrc` (or __graft_entry__.build())" % dop_path)
    dop = C.CDLL(dop_path)
    for name in DOPPLER_ABI_SYMBOLS:
        setattr(lib, name, getattr(dop, name))
    lib.fdoct_doppler_size.argtypes = [C.POINTER(_CDopplerParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fdoct_doppler.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_CDopplerParams), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int]
    lib.fdoct_process_doppler.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(_CDopplerParams),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    # include/fdoct_dispersion.h: likewise; the binding is a module of its own (fdoct_amd/dispersion.py)
    from . import dispersion
    dispersion.attach(lib)
    # include/fdoct_vibro.h: likewise (fdoct_amd/vibrometry.py)
    from . import vibrometry
    vibrometry.attach(lib)
    # include/fdoct_angio.h: likewise (fdoct_amd/angiography.py)
    from . import angiography
    angiography.attach(lib)
    # include/fdoct_cxavg.h: likewise (fdoct_amd/coherent.py)
    from . import coherent
    coherent.attach(lib)
    # include/fdoct_ssada.h: likewise (fdoct_amd/ssada.py)
    from . import ssada
    ssada.attach(lib)
    # include/fdoct_enface.h: likewise (fdoct_amd/enface.py)
    from . import enface
    enface.attach(lib)
    _lib = lib
    return lib


class PinnedArray:
    """A numpy view of pinned host memory from fdoct_host_alloc (full-speed, overlappable PCIe copies in process())."""

    def __init__(self, shape, dtype):
        self._lib = load_library()
        self.array = None
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._ptr = self._lib.fdoct_host_alloc(max(n, 1))
        if not self._ptr:
            raise FdoctError(-4, "fdoct_host_alloc(%d) failed" % n)
        buf = (C.c_char * max(n, 1)).from_address(self._ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self._ptr:
            self.array = None
            self._lib.fdoct_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        self.free()


def build_resample_table(width, multiplier, numfftpoints, lambdamin, lambdamax):
    """nearestkindex, fractionalk of BscanFFT.cpp:615-698 (host only, no device)."""
    idx = np.zeros(numfftpoints, np.int32)
    frac = np.zeros(numfftpoints, np.float64)
    rc = load_library().fdoct_build_resample_table(width, multiplier, numfftpoints, lambdamin, lambdamax,
                                                   idx.ctypes.data, frac.ctypes.data)
    if rc:
        raise FdoctError(rc, "fdoct_build_resample_table")
    return idx, frac


def build_window(width):
    """barthannwin of BscanFFT.cpp:936-944 (host only)."""
    w = np.zeros(width, np.float64)
    rc = load_library().fdoct_build_window(width, w.ctypes.data)
    if rc:
        raise FdoctError(rc, "fdoct_build_window")
    return w


def build_colormap_jet():
    """COLORMAP_JET (BscanFFT.cpp:1284) as OpenCV builds it: (256, 3) uint8, B,G,R (host only; fdoct_build_colormap_jet)."""
    t = np.zeros((256, 3), np.uint8)
    rc = load_library().fdoct_build_colormap_jet(t.ctypes.data)
    if rc:
        raise FdoctError(rc, "fdoct_build_colormap_jet")
    return t


def besseldb_inverse(y):
    """fdoct_besseldb_inverse: the reference's besseldbinverse table (BscanFFTpeak.cpp:243-395) at every y.  Needs no GPU."""
    a = np.ascontiguousarray(y, np.float64)
    out = np.empty_like(a)
    rc = load_library().fdoct_besseldb_inverse(a.ctypes.data, a.size, out.ctypes.data)
    if rc:
        raise FdoctError(rc, "fdoct_besseldb_inverse: bad arguments")
    return out


def normalize_minmax(y, lo=0.0, hi=1.0):
    """fdoct_normalize_minmax: cv::normalize(y, y, lo, hi, NORM_MINMAX) on a copy of y as float64.  Needs no GPU."""
    a = np.array(y, np.float64, order="C")
    rc = load_library().fdoct_normalize_minmax(a.ctypes.data if a.size else None, a.size, lo, hi)
    if rc:
        raise FdoctError(rc, "fdoct_normalize_minmax: bad arguments")
    return a


def colour_sum_scale():
    """fdoct_colour_sum_scale: 0.00130718954, the factor of BscanFFTwebcam.cpp:1031's channel sum.  Needs no GPU."""
    return float(load_library().fdoct_colour_sum_scale())


def bscanbin_size(depths, ascans, binx, biny, upx=None, upy=None):
    """fdoct_bscanbin_size: (out_depths, out_ascans) of the output binning; upx / upy default to binx / biny.  Needs no GPU."""
    od, oa = C.c_int(), C.c_int()
    rc = load_library().fdoct_bscanbin_size(depths, ascans, binx, biny, binx if upx is None else upx, biny if upy is None else upy,
                                            C.byref(od), C.byref(oa))
    if rc:
        raise FdoctError(rc, "fdoct_bscanbin_size: factors outside 1..16 / 1..64, or sizes they do not divide")
    return od.value, oa.value


def bscanbin_taps(up):
    """fdoct_bscanbin_taps: (taps float64 (up, 4), first source offset int32 (up,)) of INTER_CUBIC at scale 1 / up.  Needs no GPU."""
    taps = np.zeros((max(up, 0), 4), np.float64)
    off = np.zeros(max(up, 0), np.int32)
    rc = load_library().fdoct_bscanbin_taps(up, taps.ctypes.data if taps.size else None, off.ctypes.data if off.size else None)
    if rc:
        raise FdoctError(rc, "fdoct_bscanbin_taps: up must be 1..64")
    return taps, off


def manualavg_plan(manualaverages, mode, accumulated, nbscans):
    """fdoct_manualavg_plan: (emitted, accumulated afterwards) for nbscans more images.  Needs no GPU."""
    e, a = C.c_int(), C.c_int()
    rc = load_library().fdoct_manualavg_plan(manualaverages, mode, accumulated, nbscans, C.byref(e), C.byref(a))
    if rc:
        raise FdoctError(rc, "fdoct_manualavg_plan: manualaverages < 1, a bad mode, accumulated outside 0..manualaverages or nbscans < 0")
    return e.value, a.value


def doppler_params(axis, lag, win=(1, 1), bulk=None, scale=1.0, min_power=0.0):
    """fdoct_doppler_params from the binding's arguments.  bulk: None or False (no bulk-motion correction), True (every depth), or
    (first, count) depths of the bulk sum, count 0 meaning all from `first` on."""
    try:
        wa, wd = (int(w) for w in win)
    except (TypeError, ValueError):
        raise FdoctError(-1, "win is (win_ascans, win_depths)")
    if bulk is None or bulk is False:
        on, first, count = 0, 0, 0
    elif bulk is True:
        on, first, count = 1, 0, 0
    else:
        try:
            first, count = (int(b) for b in bulk)
        except (TypeError, ValueError):
            raise FdoctError(-1, "bulk is None, True or (first, count)")
        on = 1
    return _CDopplerParams(int(axis), int(lag), wa, wd, on, first, count, float(scale), float(min_power))


def doppler_size(axis, lag, nframes, ascans, depths, win=(1, 1), bulk=None, scale=1.0, min_power=0.0):
    """fdoct_doppler_size: (pair_images, pair_rows) of the pair images, or FdoctError where the parameters are refused.  Needs no GPU."""
    p = doppler_params(axis, lag, win, bulk, scale, min_power)
    pi, pr = C.c_int(), C.c_int()
    rc = load_library().fdoct_doppler_size(C.byref(p), int(nframes), int(ascans), int(depths), C.byref(pi), C.byref(pr))
    if rc:
        raise FdoctError(rc, "fdoct_doppler_size: a window outside 1..32, a lag that leaves no pair, a bulk range outside the depths, "
                             "or a scale or min_power that is not finite")
    return pi.value, pr.value


_DOPPLER_WANTS = ("phase", "corr", "power")


def _doppler_outputs(want, shape):
    """The requested result arrays of a Doppler call, in the order (phase, corr, power); None where not requested."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _DOPPLER_WANTS for w in want) or len(set(want)) != len(want):
        raise FdoctError(-1, "want names one or more of 'phase', 'corr', 'power', each once")
    outs = {w: np.empty(shape, np.complex64 if w == "corr" else np.float32) for w in want}
    return want, outs


def _frame_batch(frames):
    """Host camera frames as (array, nframes, row pitch in bytes): (nframes, rows, cols) of u8 / u16 / f32 / f64, rows contiguous;
    or (nframes, rows, cols, 3) uint8, the B,G,R frames of a handle with set_colour_input."""
    a = np.asarray(frames)
    if a.dtype not in _NP2DT:
        a = a.astype(np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim == 4:
        n, r, c, ch = a.shape
        if ch != 3 or a.dtype != np.uint8:
            raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
        if a.strides[3] != 1 or a.strides[2] != 3 or a.strides[0] != a.strides[1] * r or a.strides[1] < 3 * c:
            a = np.ascontiguousarray(a)
        return a, n, a.strides[1]
    n, r, c = a.shape
    if a.strides[2] != a.itemsize or a.strides[0] != a.strides[1] * r or a.strides[1] < c * a.itemsize:
        a = np.ascontiguousarray(a)
    return a, n, a.strides[1]


def _db_batch(db, layout):
    """A host dB batch as (array, nbscans, depths, ascans): (n, ascans, depths) row-major, (n, depths, ascans) transposed."""
    a = np.ascontiguousarray(db, np.float32)
    if a.ndim == 2:
        a = a[None]
    n, r, c = a.shape
    return (a, n, r, c) if layout == LAYOUT_TRANSPOSED else (a, n, c, r)


class Reconstructor:
    """One handle = the processing state of one acquisition loop on one GPU."""
    _roi_w = 0  # width of the peak-hold ROI set last (fdoct_set_peakhold_roi; a clone starts without one)

    def __init__(self, cfg: Config):
        self.lib = load_library()
        self.cfg = cfg
        c = _CConfig(C.sizeof(_CConfig), cfg.width, cfg.height, cfg.numfftpoints, cfg.numdisplaypoints,
                     cfg.increasefftpointsmultiplier, cfg.averages, cfg.rowwisenormalize, cfg.donotnormalize,
                     cfg.movavgn, cfg.variant, cfg.dc_mask, cfg.device, cfg.lambdamin, cfg.lambdamax)
        h = C.c_void_p()
        rc = self.lib.fdoct_create(C.byref(c), C.byref(h))
        if rc:
            raise FdoctError(rc, self.lib.fdoct_last_error(None).decode())
        self.h = h

    # -- plumbing
    def _check(self, rc):
        if rc:
            raise FdoctError(rc, self.lib.fdoct_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.fdoct_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ref(self, fn, data):
        if data is None:
            self._check(fn(self.h, None, DTYPE_F64, 0, 0))
            return
        a = np.ascontiguousarray(data)
        if a.dtype not in _NP2DT:
            a = a.astype(np.float64)
        if a.ndim == 1:
            a = a[None, :]
        self._check(fn(self.h, a.ctypes.data, _NP2DT[a.dtype], a.shape[0], a.strides[0]))

    # -- state, named after the reference's locals / key handlers
    def set_background(self, data_yb):
        self._ref(self.lib.fdoct_set_background, data_yb)

    def set_pi_frame(self, data_yp):
        self._ref(self.lib.fdoct_set_pi_frame, data_yp)

    def set_dark(self, data_yd):
        self._ref(self.lib.fdoct_set_dark, data_yd)

    def set_window(self, barthannwin):
        if barthannwin is None:
            self._check(self.lib.fdoct_set_window(self.h, None, 0))
        else:
            w = np.ascontiguousarray(barthannwin, np.float64)
            self._check(self.lib.fdoct_set_window(self.h, w.ctypes.data, w.size))

    def set_resample_table(self, nearestkindex, fractionalk):
        i = np.ascontiguousarray(nearestkindex, np.int32)
        f = np.ascontiguousarray(fractionalk, np.float64)
        self._check(self.lib.fdoct_set_resample_table(self.h, i.ctypes.data, f.ctypes.data, i.size))

    def set_lambda_range(self, lambdamin, lambdamax):
        self._check(self.lib.fdoct_set_lambda_range(self.h, lambdamin, lambdamax))

    def set_dispersion_phase(self, cos_sin_pairs):
        if cos_sin_pairs is None:
            self._check(self.lib.fdoct_set_dispersion_phase(self.h, None, 0))
        else:
            p = np.ascontiguousarray(cos_sin_pairs, np.float32)
            self._check(self.lib.fdoct_set_dispersion_phase(self.h, p.ctypes.data, p.size // 2))

    def get_resample_table(self):
        n = self.cfg.numfftpoints
        i = np.zeros(n, np.int32)
        f = np.zeros(n, np.float64)
        self._check(self.lib.fdoct_get_resample_table(self.h, i.ctypes.data, f.ctypes.data, n))
        return i, f

    def get_window(self):
        n = self.cfg.width   # W entries whatever the zero-pad multiplier is (applied before the upsampling)
        w = np.zeros(n, np.float64)
        self._check(self.lib.fdoct_get_window(self.h, w.ctypes.data, n))
        return w

    def set_stream(self, hip_stream_ptr):
        """All later work of this handle goes to that HIP stream (None: the handle's own), behind everything the handle has
        enqueued so far: an event is recorded on the stream it leaves, so that stream must still exist when this is called."""
        self._check(self.lib.fdoct_set_stream(self.h, hip_stream_ptr))

    def set_launch(self, threads_per_block=0, blocks=0):
        self._check(self.lib.fdoct_set_launch(self.h, threads_per_block, blocks))

    def set_plan(self, plan_id=-1, force_general_kernel=False):
        self._check(self.lib.fdoct_set_plan(self.h, plan_id, int(force_general_kernel)))

    def set_frontend(self, mediann=0, binx=1, biny=1):
        """medianBlur + INTER_AREA binning (BscanFFT.cpp:953-958): process() then takes RAW camera frames."""
        self._check(self.lib.fdoct_set_frontend(self.h, mediann, binx, biny))
        self._fe = (binx, biny)

    def frontend(self, raw, mediann=0, binx=1, biny=1):
        """The front end on its own: raw (nframes, h, w) u8/u16 -> binned frames (same dtype)."""
        a = np.ascontiguousarray(raw)
        if a.ndim == 2:
            a = a[None]
        n, hh, ww = a.shape
        out = np.empty((n, hh // biny, ww // binx), a.dtype)
        self._check(self.lib.fdoct_frontend(self.h, a.ctypes.data, _NP2DT[a.dtype], n, ww, hh, a.strides[1], mediann, binx, biny,
                                            out.ctypes.data))
        return out

    # -- the webcam's B,G,R frames (include/fdoct_colour.h)
    def set_colour_input(self, channelnum=-1):
        """BscanFFTwebcam.ini's channelnum: process* / capture_reference* / frame_minmax then take 8-bit (nframes, raw_h, raw_w, 3)
        B,G,R frames.  0 / 1 / 2: that channel; 3: (B + G + R) * colour_sum_scale() as doubles; -1: mono frames again."""
        self._check(self.lib.fdoct_set_colour_input(self.h, int(channelnum)))

    def get_colour_input(self):
        c = C.c_int()
        self._check(self.lib.fdoct_get_colour_input(self.h, C.byref(c)))
        return c.value

    def colour_extract(self, bgr, channelnum, mediann=0, binx=1, biny=1):
        """The colour stage on its own: bgr (nframes, raw_h, raw_w, 3) uint8 on the host (a view with padded rows passes its pitch
        on) -> (nframes, raw_h / biny, raw_w / binx) uint8 (channelnum 0-2) or float64 (3)."""
        a = np.asarray(bgr)
        if a.ndim == 3:
            a = a[None]
        a, n, pitch = _frame_batch(a)
        if a.ndim != 4:
            raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
        hh, ww = a.shape[1], a.shape[2]
        out = np.empty((n, hh // max(biny, 1), ww // max(binx, 1)), np.float64 if channelnum == 3 else np.uint8)
        self._check(self.lib.fdoct_colour_extract(self.h, a.ctypes.data, MEM_HOST, n, ww, hh, pitch, channelnum, mediann, binx, biny,
                                                  out.ctypes.data, MEM_HOST))
        return out

    def colour_extract_device(self, d_bgr_ptr, nframes, raw_w, raw_h, pitch, channelnum, d_out_ptr, mediann=0, binx=1, biny=1):
        """... on device-resident frames (raw device addresses, any alignment; the output packed).  Enqueues on the handle's stream."""
        self._check(self.lib.fdoct_colour_extract(self.h, d_bgr_ptr, MEM_DEVICE, nframes, raw_w, raw_h, pitch, channelnum, mediann,
                                                  binx, biny, d_out_ptr, MEM_DEVICE))

    # -- display post-chain (BscanFFT.cpp:1242-1255, 1284, 1225-1230)
    def set_colormap(self, bgr256=None):
        """256 x (B,G,R) uint8 table for display(colour=True); None = built-in jet."""
        if bgr256 is None:
            self._check(self.lib.fdoct_set_colormap(self.h, None))
        else:
            t = np.ascontiguousarray(bgr256, np.uint8).reshape(768)
            self._check(self.lib.fdoct_set_colormap(self.h, t.ctypes.data))

    def colormap(self):
        t = np.empty(768, np.uint8)
        self._check(self.lib.fdoct_get_colormap(self.h, t.ctypes.data))
        return t.reshape(256, 3)

    def display(self, bscandb, bscanthreshold=-30.0, clampupper=False, colour=False):
        """bscandb: float32 (nbscans, rows, cols) or (rows, cols) on the host.  Returns the u8 display image(s)
        and, with colour=True, the colour-mapped (.., 3) BGR image(s) as well."""
        a = np.ascontiguousarray(bscandb, np.float32)
        single = a.ndim == 2
        if single:
            a = a[None]
        n, r, c = a.shape
        gray = np.empty((n, r, c), np.uint8)
        bgr = np.empty((n, r, c, 3), np.uint8) if colour else None
        self._check(self.lib.fdoct_display(self.h, a.ctypes.data, MEM_HOST, n, r, c, float(bscanthreshold), int(clampupper),
                                           gray.ctypes.data, bgr.ctypes.data if colour else None, MEM_HOST))
        if single:
            gray, bgr = gray[0], (bgr[0] if colour else None)
        return (gray, bgr) if colour else gray

    def display_device(self, d_db_ptr, nbscans, rows, cols, d_gray_ptr, d_bgr_ptr=None, bscanthreshold=-30.0,
                       clampupper=False):
        """Enqueue on the handle's stream; raw device addresses."""
        self._check(self.lib.fdoct_display(self.h, d_db_ptr, MEM_DEVICE, nbscans, rows, cols, float(bscanthreshold),
                                           int(clampupper), d_gray_ptr, d_bgr_ptr, MEM_DEVICE))

    def lockin_db(self, bscan, jscan):
        """J0 lock-in: 20*ln(max(bscan - jscan, 0) + 1e-3)/2.303 for linear B-scans against one saved jscan."""
        b = np.ascontiguousarray(bscan, np.float32)
        j = np.ascontiguousarray(jscan, np.float32)
        n = b.size // j.size
        if n * j.size != b.size:
            raise ValueError("bscan must hold a whole number of jscan-sized B-scans")
        out = np.empty_like(b)
        self._check(self.lib.fdoct_lockin_db(self.h, b.ctypes.data, j.ctypes.data, MEM_HOST, n, j.size, out.ctypes.data))
        return out

    def lockin_db_device(self, d_bscan_ptr, d_jscan_ptr, nbscans, count, d_out_ptr):
        """... on device-resident B-scans of `count` floats each against one jscan (raw device addresses).  Enqueues on the handle's
        stream."""
        self._check(self.lib.fdoct_lockin_db(self.h, d_bscan_ptr, d_jscan_ptr, MEM_DEVICE, int(nbscans), int(count), d_out_ptr))

    def set_averages(self, averages):
        """Frames averaged per output B-scan from the next call on (the reference's averagestoggle)."""
        self._check(self.lib.fdoct_set_averages(self.h, int(averages)))
        self.cfg.averages = int(averages)

    def set_bandpass(self, on=True):
        """BscanDark.cpp's band-pass inside the zero-pad upsampling (needs increasefftpointsmultiplier > 1)."""
        self._check(self.lib.fdoct_set_bandpass(self.h, int(on)))

    def set_staged(self, on=True):
        """Two-kernel mode (resample stage, FFT stage) for per-stage roofline measurements."""
        self._check(self.lib.fdoct_set_staged(self.h, int(on)))

    def prepare(self, dtype=DTYPE_U16, layout=LAYOUT_ROWMAJOR):
        """Build the tables, resolve the kernel family and compile / load a run-time compiled kernel without frames
        (fdoct_prepare).  Returns KERNEL_*: what process() will take."""
        rc = self.lib.fdoct_prepare(self.h, dtype, layout)
        if rc < 0:
            self._check(rc)
        return rc

    def set_precise_division(self, on=True):
        """1/background as two floats on the fused fast path too (fdoct_set_precise_division)."""
        self._check(self.lib.fdoct_set_precise_division(self.h, int(on)))

    def set_jit(self, on=True):
        """Compile the wave-per-row kernel for this handle's geometry at run time when it is not a built-in shape (fdoct_set_jit)."""
        self._check(self.lib.fdoct_set_jit(self.h, int(on)))

    def jit_note(self):
        """Why the last run-time compile was refused ('' = nothing refused); the call itself fell back and succeeded."""
        return self.lib.fdoct_jit_note(self.h).decode()

    def last_kernel(self):
        """KERNEL_*: the kernel family the last process call launched (fdoct_last_kernel)."""
        return self.lib.fdoct_last_kernel(self.h)

    def clone_to_device(self, device):
        """A second Reconstructor with the same configuration, state and settings on another GPU of this process."""
        import dataclasses
        out = C.c_void_p()
        self._check(self.lib.fdoct_clone_to_device(self.h, device, C.byref(out)))
        r = object.__new__(Reconstructor)
        r.lib = self.lib
        r.cfg = dataclasses.replace(self.cfg, device=device)
        r.h = out
        return r

    def get_ylin(self, row0, nrows):
        """data_ylin rows of the last staged run (BscanFFTsim.cpp:901-909 dumps the first frame's): (nrows, numfftpoints)."""
        out = np.empty((nrows, self.cfg.numfftpoints), np.float64)
        self._check(self.lib.fdoct_get_ylin(self.h, row0, nrows, out.ctypes.data))
        return out

    # -- B-scan readouts (include/fdoct_roi.h).  Host batches are float32 (nbscans, ascans, depths) in the row-major layout,
    # (nbscans, depths, ascans) in the transposed one; the *_device forms take raw device addresses and enqueue.
    def ascan_minmax(self, db, ascanat, layout=LAYOUT_ROWMAJOR):
        """printMinMaxAscan (BscanFFT.cpp:146-171): per B-scan (min, max) of A-scan ascanat, depth rows 0-3 read as row 4."""
        a, n, d, h = _db_batch(db, layout)
        lo, hi = np.empty(n, np.float32), np.empty(n, np.float32)
        self._check(self.lib.fdoct_ascan_minmax(self.h, a.ctypes.data, MEM_HOST, layout, n, d, h, ascanat, lo.ctypes.data,
                                                hi.ctypes.data, MEM_HOST))
        return lo, hi

    def ascan_minmax_device(self, d_db_ptr, nbscans, depths, ascans, ascanat, d_min_ptr, d_max_ptr, layout=LAYOUT_ROWMAJOR):
        self._check(self.lib.fdoct_ascan_minmax(self.h, d_db_ptr, MEM_DEVICE, layout, nbscans, depths, ascans, ascanat,
                                                d_min_ptr, d_max_ptr, MEM_DEVICE))

    def roi_mean(self, db, ascanat, vertpos, width, layout=LAYOUT_ROWMAJOR):
        """printAvgROI (BscanFFT.cpp:99-144): per B-scan mean (float64) of depths vertpos..+2 x A-scans ascanat..+width-1."""
        a, n, d, h = _db_batch(db, layout)
        out = np.empty(n, np.float64)
        self._check(self.lib.fdoct_roi_mean(self.h, a.ctypes.data, MEM_HOST, layout, n, d, h, ascanat, vertpos, width,
                                            out.ctypes.data, MEM_HOST))
        return out

    def roi_mean_device(self, d_db_ptr, nbscans, depths, ascans, ascanat, vertpos, width, d_out_ptr, layout=LAYOUT_ROWMAJOR):
        self._check(self.lib.fdoct_roi_mean(self.h, d_db_ptr, MEM_DEVICE, layout, nbscans, depths, ascans, ascanat, vertpos,
                                            width, d_out_ptr, MEM_DEVICE))

    def set_peakhold_roi(self, x, y, w, h, ascanat):
        """The peak-hold ROI on the D x H picture (x, w: A-scans; y, h: depths) and the held A-scan; resets the column holds."""
        self._check(self.lib.fdoct_set_peakhold_roi(self.h, x, y, w, h, ascanat))
        self._roi_w = w

    def peakhold(self, slot, db, layout=LAYOUT_ROWMAJOR):
        """Folds a host dB batch into hold slot 1..4."""
        a, n, d, h = _db_batch(db, layout)
        self._check(self.lib.fdoct_peakhold(self.h, slot, a.ctypes.data, MEM_HOST, layout, n, d, h))

    def peakhold_device(self, slot, d_db_ptr, nbscans, depths, ascans, layout=LAYOUT_ROWMAJOR):
        self._check(self.lib.fdoct_peakhold(self.h, slot, d_db_ptr, MEM_DEVICE, layout, nbscans, depths, ascans))

    def peakhold_values(self, slot, roi_width=None):
        """(colmax float32[w], ascanmax float, B-scans held) of one slot; roi_width=None reads the width of the ROI set last."""
        w = self._roi_w if roi_width is None else roi_width
        cols = np.empty(w, np.float32)
        amax, count = C.c_float(), C.c_longlong()
        self._check(self.lib.fdoct_get_peakhold(self.h, slot, cols.ctypes.data if w else None, C.byref(amax), C.byref(count)))
        return cols, amax.value, count.value

    def clear_peakhold(self, slot):
        self._check(self.lib.fdoct_clear_peakhold(self.h, slot))

    def vibration(self, mode, lambda0=None):
        """(profile_nm float64[w], disp_nm, err_nm) of BscanFFTpeak's mode 3 (slots 1-3) or 4 (slots 1-4)."""
        prof = np.empty(self._roi_w, np.float64)
        disp, err = C.c_double(), C.c_double()
        self._check(self.lib.fdoct_vibration_profile(self.h, mode, -1.0 if lambda0 is None else float(lambda0),
                                                     prof.ctypes.data if prof.size else None, C.byref(disp), C.byref(err)))
        return prof, disp.value, err.value

    # -- reference frames captured from camera frames (include/fdoct_capture.h).  Host frames are (nframes, rows, cols) arrays in
    # the format process() takes (RAW camera frames when a front end is set); a view with padded rows passes its pitch on.
    def capture_reference(self, role, frames, out=False):
        """The b / p / dark key on host frames: the result becomes the handle's frame of `role` (REF_NONE: no state changes).
        out=True returns it as float64 (H, W)."""
        a, n, pitch = _frame_batch(frames)
        res = np.empty((self.cfg.height, self.cfg.width), np.float64) if out else None
        self._check(self.lib.fdoct_capture_reference(self.h, role, a.ctypes.data, _NP2DT[a.dtype], MEM_HOST, n, pitch,
                                                     res.ctypes.data if out else None))
        return res

    def capture_reference_device(self, role, d_ptr, dtype, nframes, pitch=0, out=False):
        """... on device-resident frames (raw device address)."""
        res = np.empty((self.cfg.height, self.cfg.width), np.float64) if out else None
        self._check(self.lib.fdoct_capture_reference(self.h, role, d_ptr, dtype, MEM_DEVICE, nframes, pitch,
                                                     res.ctypes.data if out else None))
        return res

    def get_reference(self, role):
        """The frame `role` holds as float64 (rows, W), rows 1 or H; None when unset."""
        rows = C.c_int()
        self._check(self.lib.fdoct_get_reference(self.h, role, None, 0, C.byref(rows)))
        if rows.value == 0:
            return None
        a = np.empty((rows.value, self.cfg.width), np.float64)
        self._check(self.lib.fdoct_get_reference(self.h, role, a.ctypes.data, a.size, C.byref(rows)))
        return a

    def frame_minmax(self, frames):
        """"Max intensity" (BscanFFT.cpp:1105-1108): (min, max) float64[nframes] of every frame after the front end."""
        a, n, pitch = _frame_batch(frames)
        lo, hi = np.empty(n, np.float64), np.empty(n, np.float64)
        self._check(self.lib.fdoct_frame_minmax(self.h, a.ctypes.data, _NP2DT[a.dtype], MEM_HOST, n, pitch, lo.ctypes.data,
                                                hi.ctypes.data, MEM_HOST))
        return lo, hi

    def frame_minmax_device(self, d_ptr, dtype, nframes, pitch, d_min_ptr, d_max_ptr):
        self._check(self.lib.fdoct_frame_minmax(self.h, d_ptr, dtype, MEM_DEVICE, nframes, pitch, d_min_ptr, d_max_ptr, MEM_DEVICE))

    # -- BscanDark's lpfilter and the capture's options (include/fdoct_lowpass.h)
    def set_capture_options(self, lowpass=False, raw_accumulate=False):
        """BscanDark.ini's lowpassfilter (lpfilter ends the capture of BACKGROUND / DARK / NONE) and saveinterferograms (the
        capture skips the moving average)."""
        self._check(self.lib.fdoct_set_capture_options(self.h, int(bool(lowpass)), int(bool(raw_accumulate))))

    def get_capture_options(self):
        """(lowpass, raw_accumulate) as bools."""
        lp, raw = C.c_int(), C.c_int()
        self._check(self.lib.fdoct_get_capture_options(self.h, C.byref(lp), C.byref(raw)))
        return bool(lp.value), bool(raw.value)

    def lowpass_rows(self, rows, out=None):
        """lpfilter (BscanDark.cpp:119-167) on a float64 (rows, width) array, or one row, in host memory.  Returns a new array;
        or filters into `out`, which has the rows' shape and strides (a view with padded rows passes its pitch on) and may be
        `rows` itself."""
        a = np.asarray(rows)
        if out is None:
            a = np.ascontiguousarray(a)
            out = np.empty_like(a)
        if a.dtype != np.float64 or a.ndim not in (1, 2) or a.size == 0 or a.strides[-1] != 8:
            raise FdoctError(-1, "lowpass_rows takes float64 rows of contiguous samples")
        if out.dtype != np.float64 or out.shape != a.shape or out.strides != a.strides:
            raise FdoctError(-1, "out must be float64 of the rows' shape and strides")
        nrows, width = (1, a.shape[0]) if a.ndim == 1 else a.shape
        pitch = a.strides[0] if a.ndim == 2 and nrows > 1 else 0
        self._check(self.lib.fdoct_lowpass_rows(self.h, a.ctypes.data, MEM_HOST, nrows, width, pitch, out.ctypes.data, MEM_HOST))
        return out

    def lowpass_rows_device(self, d_in_ptr, rows, width, pitch=0, d_out_ptr=None):
        """... on device-resident rows (raw device addresses; d_out_ptr None: in place).  Enqueues on the handle's stream."""
        self._check(self.lib.fdoct_lowpass_rows(self.h, d_in_ptr, MEM_DEVICE, rows, width, pitch,
                                                d_in_ptr if d_out_ptr is None else d_out_ptr, MEM_DEVICE))

    # -- BscanDark's calibration on the device (include/fdoct_calibrate.h)
    def normalize_rows_minmax(self, rows, lo=0.0001, hi=1.0, per_row=True, out=None):
        """cv::normalize(.., lo, hi, NORM_MINMAX) on a float64 (rows, width) array, or one row, in host memory: every row on its
        own (per_row, normalizerows) or the array as one plane.  Returns a new array; or normalises into `out`, which has the rows'
        shape and strides (a view with padded rows passes its pitch on) and may be `rows` itself."""
        a = np.asarray(rows)
        if out is None:
            a = np.ascontiguousarray(a)
            out = np.empty_like(a)
        if a.dtype != np.float64 or a.ndim not in (1, 2) or a.size == 0 or a.strides[-1] != 8:
            raise FdoctError(-1, "normalize_rows_minmax takes float64 rows of contiguous samples")
        if out.dtype != np.float64 or out.shape != a.shape or out.strides != a.strides:
            raise FdoctError(-1, "out must be float64 of the rows' shape and strides")
        nrows, width = (1, a.shape[0]) if a.ndim == 1 else a.shape
        pitch = a.strides[0] if a.ndim == 2 and nrows > 1 else 0
        self._check(self.lib.fdoct_normalize_rows_minmax(self.h, a.ctypes.data, MEM_HOST, nrows, width, pitch, float(lo), float(hi),
                                                         int(bool(per_row)), out.ctypes.data, MEM_HOST))
        return out

    def normalize_rows_minmax_device(self, d_ptr, rows, width, pitch=0, lo=0.0001, hi=1.0, per_row=True, d_out_ptr=None):
        """... on device-resident rows (raw device addresses; d_out_ptr None: in place).  Enqueues on the handle's stream."""
        self._check(self.lib.fdoct_normalize_rows_minmax(self.h, d_ptr, MEM_DEVICE, rows, width, pitch, float(lo), float(hi),
                                                         int(bool(per_row)), d_ptr if d_out_ptr is None else d_out_ptr, MEM_DEVICE))

    def calibrate_capture(self, slot, frames, out=False):
        """One of BscanDark's captures (CAL_DARK / CAL_REFERENCE / CAL_SAMPLE) on host frames: accumulated, normalised and
        filtered on the device and held there; CAL_DARK also becomes the handle's dark frame.  out=True returns the result as
        float64 (H, W) -- for the reference and sample slots that is the call's only download."""
        if slot not in (CAL_DARK, CAL_REFERENCE, CAL_SAMPLE):
            raise FdoctError(-1, "calibrate_capture: slot is CAL_DARK, CAL_REFERENCE or CAL_SAMPLE")
        a, n, pitch = _frame_batch(frames)
        res = np.empty((self.cfg.height, self.cfg.width), np.float64) if out else None
        self._check(self.lib.fdoct_calibrate_capture(self.h, slot, a.ctypes.data, _NP2DT[a.dtype], MEM_HOST, n, pitch,
                                                     res.ctypes.data if out else None))
        return res

    def calibrate_capture_device(self, slot, d_ptr, dtype, nframes, pitch=0, out=False):
        """... on device-resident frames (raw device address)."""
        if slot not in (CAL_DARK, CAL_REFERENCE, CAL_SAMPLE):
            raise FdoctError(-1, "calibrate_capture_device: slot is CAL_DARK, CAL_REFERENCE or CAL_SAMPLE")
        res = np.empty((self.cfg.height, self.cfg.width), np.float64) if out else None
        self._check(self.lib.fdoct_calibrate_capture(self.h, slot, d_ptr, dtype, MEM_DEVICE, nframes, pitch,
                                                     res.ctypes.data if out else None))
        return res

    def calibrate_compose(self, out=False):
        """BscanDark.cpp:996 from the three held captures, (yr - yd) + (ys - yd): the result becomes the handle's background.
        out=True returns it as float64 (H, W)."""
        res = np.empty((self.cfg.height, self.cfg.width), np.float64) if out else None
        self._check(self.lib.fdoct_calibrate_compose(self.h, res.ctypes.data if out else None))
        return res

    def calibrate_state(self):
        """(dark, reference, sample) as bools: which captures the handle holds."""
        held = (C.c_int * 3)()
        self._check(self.lib.fdoct_calibrate_state(self.h, held))
        return tuple(bool(x) for x in held)

    def calibrate_clear(self):
        """Drops the three held captures; the handle's dark frame and background stay."""
        self._check(self.lib.fdoct_calibrate_clear(self.h))

    # -- spinjnt's output binning (include/fdoct_bscanbin.h).  Host batches are float32 like the readouts'.
    def bscan_bin(self, bscan, binx, biny, upx=None, upy=None, multiplyfactor=None, jscan=None, layout=LAYOUT_ROWMAJOR,
                  want_db=True, want_bscan=True):
        """BscanFFTspinjnt.cpp:1856-1874 on host B-scans: INTER_AREA by binx x biny, INTER_CUBIC back up by upx x upy (defaults
        binx, biny) of multiplyfactor (default binx * biny) times the binned image, and the dB of the result.  Returns
        (bscan, bscandb) float32 in the input's layout (None when not requested); a 2-D input gives 2-D results."""
        single = np.ndim(bscan) == 2
        a, n, d, h = _db_batch(bscan, layout)
        upx, upy = binx if upx is None else upx, biny if upy is None else upy
        mf = float(binx * biny) if multiplyfactor is None else float(multiplyfactor)
        od, oa = bscanbin_size(d, h, binx, biny, upx, upy)
        shp = (n, od, oa) if layout == LAYOUT_TRANSPOSED else (n, oa, od)
        j = None
        if jscan is not None:
            j = np.ascontiguousarray(jscan, np.float32)
            if j.shape != a.shape[1:]:
                raise FdoctError(-1, "jscan must be one image of the B-scans' shape")
        lin = np.empty(shp, np.float32) if want_bscan else None
        db = np.empty(shp, np.float32) if want_db else None
        self._check(self.lib.fdoct_bscan_bin(self.h, a.ctypes.data, None if j is None else j.ctypes.data, MEM_HOST, layout, n, d, h,
                                             binx, biny, upx, upy, mf, None if lin is None else lin.ctypes.data,
                                             None if db is None else db.ctypes.data, MEM_HOST))
        if single:
            lin, db = (None if lin is None else lin[0]), (None if db is None else db[0])
        return lin, db

    def bscan_bin_device(self, d_bscan_ptr, nbscans, depths, ascans, binx, biny, d_out_bscan_ptr, d_out_db_ptr, upx=None, upy=None,
                         multiplyfactor=None, d_jscan_ptr=None, layout=LAYOUT_ROWMAJOR):
        """... on device-resident B-scans (raw device addresses; either output may be None).  Enqueues on the handle's stream."""
        self._check(self.lib.fdoct_bscan_bin(self.h, d_bscan_ptr, d_jscan_ptr, MEM_DEVICE, layout, nbscans, depths, ascans, binx, biny,
                                             binx if upx is None else upx, biny if upy is None else upy,
                                             float(binx * biny) if multiplyfactor is None else float(multiplyfactor),
                                             d_out_bscan_ptr, d_out_db_ptr, MEM_DEVICE))

    # -- manual averaging of B-scans (include/fdoct_manualavg.h): an accumulator of doubles on the device, with state across calls
    def manualavg_begin(self, manualaverages, count, mode=MANUALAVG_REFERENCE):
        """manualaccum = zeros, manualaccumcount = 0 (BscanFFT.cpp:933, 567) for images of `count` floats (depths * ascans).
        MANUALAVG_REFERENCE drops the image that arrives when manualaverages are in, as the reference does; MANUALAVG_KEEP_ALL
        emits with the last of them."""
        self._check(self.lib.fdoct_manualavg_begin(self.h, int(manualaverages), int(count), int(mode)))

    def manualavg_state(self, partial=False):
        """(manualaverages, count, mode, accumulated) and, with partial=True, the running sums as float64[count] as well."""
        m, n, mode, acc = C.c_int(), C.c_size_t(), C.c_int(), C.c_int()
        self._check(self.lib.fdoct_manualavg_state(self.h, C.byref(m), C.byref(n), C.byref(mode), C.byref(acc), None))
        if not partial:
            return m.value, n.value, mode.value, acc.value
        sums = np.empty(n.value, np.float64)
        self._check(self.lib.fdoct_manualavg_state(self.h, None, None, None, None, sums.ctypes.data))
        return m.value, n.value, mode.value, acc.value, sums

    def manualavg_add(self, bscans, want_mean=True, want_db=True):
        """BscanFFT.cpp:1399-1444 for host B-scans, in order: float32 (nbscans, ...) images of the accumulator's size, or one
        such image.  Returns (mean, db) float32, each (emitted,) + the image's shape (None when not requested): mean is
        manualaccum / manualaverages, db is 20 ln(that) / 2.303."""
        a = np.ascontiguousarray(bscans, np.float32)
        m, count, mode, acc = self.manualavg_state()
        if a.size == count and (a.ndim < 2 or a.shape[0] != 1):
            a = a[None]
        n, shape = a.shape[0], a.shape[1:]
        if a.ndim < 2 or n < 1 or a.size != n * count:
            raise FdoctError(-1, "manualavg_add takes images of the accumulator's %d floats" % count)
        e = manualavg_plan(m, mode, acc, n)[0]
        mean = np.empty((e,) + shape, np.float32) if want_mean else None
        db = np.empty((e,) + shape, np.float32) if want_db else None
        got = C.c_int()
        self._check(self.lib.fdoct_manualavg_add(self.h, a.ctypes.data, MEM_HOST, n, mean.ctypes.data if want_mean and e else None,
                                                 db.ctypes.data if want_db and e else None, MEM_HOST, e, C.byref(got)))
        assert got.value == e
        return mean, db

    def manualavg_add_device(self, d_bscans_ptr, nbscans, d_mean_ptr, d_db_ptr, out_capacity):
        """... on device-resident B-scans (raw device addresses; either output may be None, both only on a call that emits
        nothing).  Enqueues on the handle's stream; returns the number of slots the call writes."""
        got = C.c_int()
        self._check(self.lib.fdoct_manualavg_add(self.h, d_bscans_ptr, MEM_DEVICE, int(nbscans), d_mean_ptr, d_db_ptr, MEM_DEVICE,
                                                 int(out_capacity), C.byref(got)))
        return got.value

    def manualavg_end(self):
        """Frees the accumulator (close() does so too)."""
        self._check(self.lib.fdoct_manualavg_end(self.h))

    # -- per-frame saves while averaging (include/fdoct_saveframes.h)
    def set_raw_magnitudes(self, on=True):
        """The chain writes a group's mean magnitude without its epsilon (with averages = 1: a frame's own magnitudes, what
        saveframes() takes); process* then refuse a dB output."""
        self._check(self.lib.fdoct_set_raw_magnitudes(self.h, int(on)))

    def get_raw_magnitudes(self):
        rc = self.lib.fdoct_get_raw_magnitudes(self.h)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def saveframes(self, frames, averages=0, in_layout=LAYOUT_ROWMAJOR, out_layout=LAYOUT_TRANSPOSED, want_gray=True,
                   want_bscan=True, want_db=True):
        """BscanFFT.cpp:1197-1240 and 1360-1377 on host magnitudes: float32 (nframes, ascans, depths) in the row-major layout,
        (nframes, depths, ascans) in the transposed one, or one such image.  Returns (gray, bscan, bscandb): gray uint8
        (nframes, depths, ascans), every frame's save picture; bscan / bscandb float32, one image per group of `averages`
        frames in out_layout.  averages = 0: no fold, both are None; so is whatever is not wanted."""
        a, n, d, h = _db_batch(frames, in_layout)
        g = n // averages if averages > 0 else 0
        shp = (g, d, h) if out_layout == LAYOUT_TRANSPOSED else (g, h, d)
        gray = np.empty((n, d, h), np.uint8) if want_gray else None
        bscan = np.empty(shp, np.float32) if want_bscan and averages > 0 else None
        db = np.empty(shp, np.float32) if want_db and averages > 0 else None
        self._check(self.lib.fdoct_saveframes(self.h, a.ctypes.data, MEM_HOST, in_layout, n, d, h,
                                              None if gray is None else gray.ctypes.data, int(averages),
                                              None if bscan is None else bscan.ctypes.data, None if db is None else db.ctypes.data,
                                              out_layout, MEM_HOST))
        return gray, bscan, db

    def saveframes_device(self, d_frames_ptr, nframes, depths, ascans, d_gray_ptr, averages=0, d_bscan_ptr=None, d_db_ptr=None,
                          in_layout=LAYOUT_ROWMAJOR, out_layout=LAYOUT_TRANSPOSED):
        """... on device-resident magnitudes (raw device addresses; the picture and the fold outputs may each be None, not all
        of them).  Enqueues on the handle's stream."""
        self._check(self.lib.fdoct_saveframes(self.h, d_frames_ptr, MEM_DEVICE, in_layout, int(nframes), int(depths), int(ascans),
                                              d_gray_ptr, int(averages), d_bscan_ptr, d_db_ptr, out_layout, MEM_DEVICE))

    # -- work
    def _out_shape(self, nframes, layout):
        g = nframes // self.cfg.averages
        if layout == LAYOUT_TRANSPOSED:
            return (g, self.cfg.numdisplaypoints, self.cfg.height)
        return (g, self.cfg.height, self.cfg.numdisplaypoints)

    def process(self, frames, want_db=True, want_bscan=True, layout=LAYOUT_ROWMAJOR, out_bscan=None, out_db=None):
        """frames: numpy (nframes, H, W) u8/u16/f32/f64 on the host -- with set_colour_input, (nframes, raw_h, raw_w, 3) uint8.  Returns (bscan, bscandb)
        float32 arrays (None when not requested).  PCIe-inclusive, synchronous.  out_bscan / out_db: caller-owned
        float32 result arrays (e.g. PinnedArray(...).array) instead of fresh ones -- a loop should pass them: a fresh
        array's first-touch page faults cost a 64-frame call four fifths of its rate (profiles/r06_pcie_rate.txt)."""
        a = np.ascontiguousarray(frames)
        if a.ndim == 2:
            a = a[None]
        if a.dtype not in _NP2DT:
            raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
        if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
            raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
        nframes = a.shape[0]
        shp = self._out_shape(nframes, layout)
        def _result(given, want):
            if given is not None:
                if given.dtype != np.float32 or given.shape != shp or not given.flags.c_contiguous:
                    raise FdoctError(-1, "result array must be C-contiguous float32 of shape %s" % (shp,))
                return given
            return np.empty(shp, np.float32) if want else None
        bscan = _result(out_bscan, want_bscan)
        db = _result(out_db, want_db)
        want_bscan, want_db = bscan is not None, db is not None
        self._check(self.lib.fdoct_process(self.h, a.ctypes.data, _NP2DT[a.dtype], MEM_HOST, nframes, a.strides[1],
                                           bscan.ctypes.data if want_bscan else None,
                                           db.ctypes.data if want_db else None, MEM_HOST, layout))
        return bscan, db

    def process_device(self, d_frames_ptr, dtype, nframes, pitch_bytes, d_bscan_ptr, d_db_ptr,
                       layout=LAYOUT_ROWMAJOR):
        """Enqueue on the handle's stream; pointers are raw device addresses (e.g. tensor.data_ptr())."""
        self._check(self.lib.fdoct_process_async(self.h, d_frames_ptr, dtype, nframes, pitch_bytes, d_bscan_ptr,
                                                 d_db_ptr, layout))

    def process_complex(self, frames, layout=LAYOUT_ROWMAJOR, out=None):
        """The complex A-scans of `frames` (numpy, as process() takes them): fdoct_process_complex.  Returns complex64 of shape
        (nframes, H, D), or (nframes, D, H) in the transposed layout: X[b] of every frame's every A-scan, unscaled; its modulus is
        what process() gives with raw magnitudes.  `averages` must be 1.  PCIe-inclusive, synchronous.  out: a caller-owned
        C-contiguous complex64 array of that shape instead of a fresh one."""
        a = np.ascontiguousarray(frames)
        if a.ndim == 2:
            a = a[None]
        if a.dtype not in _NP2DT:
            raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
        if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
            raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
        n, h, d = a.shape[0], self.cfg.height, self.cfg.numdisplaypoints
        shp = (n, d, h) if layout == LAYOUT_TRANSPOSED else (n, h, d)
        if out is None:
            out = np.empty(shp, np.complex64)
        elif out.dtype != np.complex64 or out.shape != shp or not out.flags.c_contiguous:
            raise FdoctError(-1, "result array must be C-contiguous complex64 of shape %s" % (shp,))
        self._check(self.lib.fdoct_process_complex(self.h, a.ctypes.data, _NP2DT[a.dtype], MEM_HOST, n, a.strides[1], out.ctypes.data,
                                                   MEM_HOST, layout))
        return out

    def process_complex_device(self, d_frames_ptr, dtype, nframes, pitch_bytes, d_out_ptr, layout=LAYOUT_ROWMAJOR):
        """... on device-resident frames into nframes * H * D (re, im) float pairs of device memory (raw addresses, d_out_ptr aligned
        to 8 bytes).  Enqueues on the handle's stream."""
        self._check(self.lib.fdoct_process_complex(self.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), d_out_ptr,
                                                   MEM_DEVICE, layout))

    def doppler(self, X, axis, lag, win=(1, 1), bulk=None, scale=1.0, min_power=0.0, want=("phase", "corr", "power")):
        """Phase-resolved Doppler of complex A-scans (include/fdoct_doppler.h): X is complex64 (n, H, D) on the host, row-major as
        process_complex returns it; axis DOPPLER_ASCANS or DOPPLER_FRAMES; win = (win_ascans, win_depths).  Returns the arrays `want`
        names, in its order (one name: that array alone): phase and power float32, corr complex64, all (pair_images, pair_rows, D).
        Synchronous."""
        a = np.asarray(X)
        if a.dtype != np.complex64 or a.ndim != 3:
            raise FdoctError(-1, "X must be complex64 of shape (nframes, ascans, depths)")
        a = np.ascontiguousarray(a)
        n, rows, d = a.shape
        p = doppler_params(axis, lag, win, bulk, scale, min_power)
        pi, pr = doppler_size(axis, lag, n, rows, d, win, bulk, scale, min_power)
        names, outs = _doppler_outputs(want, (pi, pr, d))
        ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
        self._check(self.lib.fdoct_doppler(self.h, a.ctypes.data, MEM_HOST, n, rows, d, C.byref(p), ptr("phase"), ptr("corr"), ptr("power"),
                                           MEM_HOST))
        return outs[names[0]] if isinstance(want, str) else tuple(outs[w] for w in names)

    def doppler_device(self, d_re_im_ptr, nframes, ascans, depths, axis, lag, d_phase_ptr, d_corr_ptr, d_power_ptr, win=(1, 1), bulk=None,
                       scale=1.0, min_power=0.0):
        """... on device-resident pairs into device memory (raw addresses; any output may be None, d_corr_ptr aligned to 8 bytes).
        Enqueues on the handle's stream."""
        p = doppler_params(axis, lag, win, bulk, scale, min_power)
        self._check(self.lib.fdoct_doppler(self.h, d_re_im_ptr, MEM_DEVICE, int(nframes), int(ascans), int(depths), C.byref(p), d_phase_ptr,
                                           d_corr_ptr, d_power_ptr, MEM_DEVICE))

    def process_doppler(self, frames, axis, lag, win=(1, 1), bulk=None, scale=1.0, min_power=0.0, want=("phase", "corr", "power")):
        """fdoct_process_doppler: process_complex's chain on `frames` (numpy, as process() takes them) followed by doppler() on the card;
        the complex A-scans never reach the host.  `averages` must be 1.  Returns what doppler() returns.  Synchronous."""
        a = np.ascontiguousarray(frames)
        if a.ndim == 2:
            a = a[None]
        if a.dtype not in _NP2DT:
            raise FdoctError(-1, "unsupported frame dtype %s" % a.dtype)
        if a.ndim == 4 and (a.shape[3] != 3 or a.dtype != np.uint8):
            raise FdoctError(-1, "colour frames are (nframes, rows, cols, 3) uint8")
        n, h, d = a.shape[0], self.cfg.height, self.cfg.numdisplaypoints
        p = doppler_params(axis, lag, win, bulk, scale, min_power)
        pi, pr = doppler_size(axis, lag, n, h, d, win, bulk, scale, min_power)
        names, outs = _doppler_outputs(want, (pi, pr, d))
        ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
        self._check(self.lib.fdoct_process_doppler(self.h, a.ctypes.data, _NP2DT[a.dtype], MEM_HOST, n, a.strides[1], C.byref(p), ptr("phase"),
                                                   ptr("corr"), ptr("power"), MEM_HOST))
        return outs[names[0]] if isinstance(want, str) else tuple(outs[w] for w in names)

    def process_doppler_device(self, d_frames_ptr, dtype, nframes, pitch_bytes, axis, lag, d_phase_ptr, d_corr_ptr, d_power_ptr, win=(1, 1),
                               bulk=None, scale=1.0, min_power=0.0):
        """... on device-resident frames into device memory (raw addresses; any output may be None).  Enqueues on the handle's stream."""
        p = doppler_params(axis, lag, win, bulk, scale, min_power)
        self._check(self.lib.fdoct_process_doppler(self.h, d_frames_ptr, dtype, MEM_DEVICE, int(nframes), int(pitch_bytes), C.byref(p),
                                                   d_phase_ptr, d_corr_ptr, d_power_ptr, MEM_DEVICE))

    def set_timing(self, on=True):
        """Device-side timing events for process_device() (process() always has them); see fdoct_set_timing."""
        self._check(self.lib.fdoct_set_timing(self.h, int(on)))

    def set_host_staging(self, threads=-1):
        """Pageable host buffers through the handle's pinned staging slots (see fdoct_set_host_staging): -1 default, 0 off, n threads."""
        self._check(self.lib.fdoct_set_host_staging(self.h, int(threads)))

    def host_staging_threads(self):
        """Copy threads a pageable batch would be staged with under the current setting (0: handed to the runtime as it is)."""
        n = self.lib.fdoct_get_host_staging(self.h)
        if n < 0:
            self._check(n)
        return n

    def synchronize(self):
        self._check(self.lib.fdoct_synchronize(self.h))

    def timing(self):
        t = _CTiming()
        self._check(self.lib.fdoct_get_timing(self.h, C.byref(t)))
        return {"process_ms": t.last_process_ms, "kernel_ms": t.last_kernel_ms,
                "resample_stage_ms": t.resample_stage_ms, "fft_stage_ms": t.fft_stage_ms, "ascans": t.ascans,
                "bytes_in": t.bytes_in, "bytes_out": t.bytes_out}

    def broadcast_state_rccl(self, nccl_comm, root=0):
        """Set-up broadcast over a caller-owned RCCL communicator (an ncclComm_t as an integer / c_void_p): fdoct_broadcast_state_rccl."""
        self._check(self.lib.fdoct_broadcast_state_rccl(self.h, C.c_void_p(nccl_comm), int(root)))

    def export_state(self):
        used = C.c_size_t()
        self._check(self.lib.fdoct_export_state(self.h, None, 0, C.byref(used)))
        buf = np.zeros(used.value, np.uint8)
        self._check(self.lib.fdoct_export_state(self.h, buf.ctypes.data, buf.size, C.byref(used)))
        return buf

    def import_state(self, blob):
        b = np.ascontiguousarray(blob, np.uint8)
        self._check(self.lib.fdoct_import_state(self.h, b.ctypes.data, b.size))
