"""The catalogue of tests/test_gpu_stream_order.py as plain Python: which Reconstructor methods enqueue on device memory (ENTRIES),
which change a handle's state (SETTERS), which public methods of either name pattern are left out and why (EXEMPT), and the pairs of
calls of which the second outgrows a handle-owned workspace the first is still using (GROWTH), with the workspace's size restated from
its `.reserve(` site.  tests/test_stream_cases.py holds the catalogue to fdoct_amd.capi.Reconstructor on the CPU -- a new `*_device`
or `set_*` method fails there until it is listed -- and every pair to "the second call needs strictly more bytes"; the GPU tests run
one case per name and fail on a name without a case.

The stream-order contract the GPU tests hold ("Stream order"): calls of one handle run in call order; a setter takes
effect for later calls only; a call with a host-memory argument returns drained; set_stream orders the new stream behind the old."""
import collections

import degenerate_cases as dg

# ---- entries: methods that enqueue work on device-resident arguments ---------------------------------------------------------------
ENTRIES = [
    "process_device", "process_complex_device", "process_doppler_device", "doppler_device", "colour_extract_device", "display_device",
    "ascan_minmax_device", "roi_mean_device", "peakhold_device", "capture_reference_device", "frame_minmax_device",
    "lowpass_rows_device", "normalize_rows_minmax_device", "calibrate_capture_device", "bscan_bin_device", "manualavg_add_device",
    "saveframes_device",
    # enqueue a memset on the handle's stream
    "manualavg_begin", "set_peakhold_roi", "clear_peakhold",
    "lockin_db_device",
    # no *_device form: the front end takes host memory only
    "frontend",
]
# entries that hand a result back in host memory and therefore return drained: the stall is over when they return, by contract
DRAINING_ENTRIES = ["capture_reference_device", "calibrate_capture_device", "frontend"]

# ---- setters: methods after which a later call must see the new state and an earlier one the old ------------------------------------
SETTERS = [
    "set_background", "set_pi_frame", "set_dark", "set_window", "set_resample_table", "set_lambda_range", "set_dispersion_phase",
    "set_averages", "set_bandpass", "set_precise_division", "set_plan", "set_staged", "set_jit", "set_launch", "set_frontend",
    "set_colour_input", "set_raw_magnitudes", "set_colormap", "set_peakhold_roi", "import_state", "capture_reference_device",
    "calibrate_compose", "manualavg_begin",
    "bscan_bin_device",   # the bin factors are arguments, but a new factor re-uploads the handle's tap table (fdoct_bscanbin.cpp)
]
# the setters that rebuild device tables, run on one handle of each table set
TABLE_SETTERS = ["set_background", "set_pi_frame", "set_dark", "set_window", "set_resample_table", "set_lambda_range", "set_dispersion_phase"]
TABLE_SETS = {   # name -> (family of degenerate_cases, background kind the handle starts with)
    "fused, 512-point plan": ("fused fast path, 512-point plan", "clean"),
    "fused, H x W background": ("fused fast path, 1024-point plan", "full"),
    "wave-per-row, built in, 160 x 4": ("wave-per-row, 160 x 4", "clean"),
    "wave-per-row, run-time compiled, 200 x 4": ("wave-per-row, run-time compiled, 200 x 4", "clean"),
    "workgroup-per-row, 2048 -> 2002": ("workgroup-per-row, 2048 -> 2002", "clean"),
    "long rows, 2048 x 8": ("long rows, 2048 x 8", "clean"),
}

# ---- public methods named *_device or set_* that are in neither list ---------------------------------------------------------------
EXEMPT = {
    "set_stream": "the subject of the stream-switch tests, not a state change of its own",
    "set_timing": "host flag: whether process_device records events; no device state",
    "set_host_staging": "host flag: copy threads of the synchronous fdoct_process pipeline; no device state",
    "set_capture_options": "read by the capture entry points alone, and those return drained",
    "clone_to_device": "makes a second handle from host state; enqueues nothing on this one",
}


def public_methods(cls):
    return sorted(n for n, v in vars(cls).items() if callable(v) and not n.startswith("_"))


def must_be_listed(cls):
    """The public methods the catalogue has to account for: every *_device and every set_*."""
    return [n for n in public_methods(cls) if n.endswith("_device") or n.startswith("set_")]


# ---- growth pairs -----------------------------------------------------------------------------------------------------------------------
# One per handle-owned workspace that grows by free and malloc (Buffer::reserve, fdoct_ctx.h) while an earlier call may still use it.
# `small` and `large` are the arguments that differ between call A and call B; `need(args)` is the workspace's size in bytes for them,
# restated from the reserve site named in `site`.
SIDE = dict(W=64, H=8, N=64, D=32)    # the side stages' handle (tests/test_gpu_staging.py's shape)
GENERIC = dg.family("workgroup-per-row, 2048 -> 2002")
STAGED = dg.family("fused, staged")
LONG = dg.family("long rows, 2048 x 8")
FAST = dg.family("fused fast path, 1024-point plan")

SF_CHUNK, SF_MAX_PARTS = 256 * 16, 256       # fdoct_saveframes.hip
DISP_CHUNK, DISP_MAX_PARTS = 256 * 16, 256   # fdoct_display.hip: display_parts
MINMAX_PARTS = 16                            # fdoct_prepass_kernels.inc
CAL_RUN, CAL_MIN_RUNS = 2, 4                 # fdoct_calibrate.hip
BIG_BUDGET = 2 << 30                         # fdoct_big_plan.h: kBigChunkBudget
LOWPASS_LONG_W = 5850                        # the first width whose bins leave LDS (stage_grid_sizes.LOWPASS_EXPECT)


def _pitch16(n_bytes):
    return (n_bytes + 15) & ~15               # frontend_pitch (fdoct_route_value.h)


def _geo(fam):
    g = fam.geometry
    return g["width"], fam.H, g["numfftpoints"], g["numdisplaypoints"]


def need_ylin(a):          # fdoct_route.cpp, launch_family_fused: in_rows * plan.NC float2, NC = N / 2 on the real path
    W, H, N, D = _geo(STAGED)
    return a["nframes"] * H * (N // 2) * 8


def need_cx(a):            # fdoct_complex.cpp: nframes * H * D pairs, the D x H layout only
    W, H, N, D = _geo(GENERIC)
    return a["nframes"] * H * D * 8


def need_dop_bulk(a):      # fdoct_doppler.cpp: pair_images * pair_rows float2; between A-scans, lag 1: nframes x (ascans - 1)
    return a["nframes"] * (SIDE["H"] - 1) * 8


def need_sim(a):           # fdoct_capi.cpp, sim_last_frames: the last frame of every group of `averages`, at the caller's pitch
    W, H, N, D = _geo(GENERIC)
    return (a["nframes"] // 2) * H * W * 2


def need_front(a):         # fdoct_route.cpp, run_frontend: binned frames of 16-byte-pitched rows (2 x 2 binning of u16)
    W, H, N, D = _geo(GENERIC)
    return _pitch16(W * 2) * H * a["nframes"]


def need_med(a):           # ... and the median's full-resolution output in front of them (no binning here)
    W, H, N, D = _geo(GENERIC)
    return _pitch16(W * 2) * H * a["nframes"]


def need_tr(a):            # fdoct_route.cpp, enqueue_one: both row-major images of the transpose pass
    W, H, N, D = _geo(GENERIC)
    return a["nframes"] * H * D * 4 * 2


def need_minmax(a):        # fdoct_route.cpp, begin_call: nframes results and nframes * MINMAX_PARTS partials, float2
    return (a["nframes"] + a["nframes"] * MINMAX_PARTS) * 8


def need_big_y(a):         # fdoct_big_host.cpp, run_big: rows of a chunk x W floats (ws_big_a / ws_big_b: the same rows x lmax pairs)
    W, H, N, D = _geo(LONG)
    lmax = max(N, W * LONG.geometry["increasefftpointsmultiplier"])
    per_group = H * (W * 4 + 2 * lmax * 8)
    groups = max(1, min(BIG_BUDGET // per_group, a["nframes"]))
    return groups * H * W * 4


def need_sf_part(a):       # fdoct_saveframes.cpp: nframes * parts (min, max) pairs of doubles, pictures only
    count = SIDE["H"] * SIDE["D"]
    parts = min(-(-count // SF_CHUNK), SF_MAX_PARTS)
    return a["nframes"] * parts * 2 * 8


def need_lp_bins(a):       # fdoct_lowpass.hip, lowpass_shape: blocks * 4 * f doubles once the bins leave LDS; blocks = rows below the cap
    import stage_grid_sizes as sg
    f, G, L, lds, staged = sg.lowpass_shape(LOWPASS_LONG_W)
    assert not staged and a["rows"] <= sg.resident(64)
    return a["rows"] * 4 * f * 8


def need_cal_mm(a):        # fdoct_calibrate.hip, minmax_shape: 2 * groups * S + 2 * groups doubles; per row, one segment a short row
    cpr = -(-SIDE["W"] // CAL_RUN)
    T = 1
    while T < min(cpr, 64):
        T *= 2
    assert -(-cpr // (CAL_MIN_RUNS * T)) == 1     # `worth` = 1: S = 1
    return (2 * a["rows"] + 2 * a["rows"]) * 8


def need_disp_part(a):     # fdoct_capi.cpp, fdoct_display: nbscans * display_parts(count) (min, max) pairs of doubles
    count = 6 * 7
    parts = max(1, min(-(-count // DISP_CHUNK), DISP_MAX_PARTS))
    return a["nbscans"] * parts * 2 * 8


def need_mov(a):           # fdoct_route.cpp, run_passes_in_front: one f32 plane of packed rows (movavgn on u16 frames)
    W, H, N, D = _geo(GENERIC)
    return a["nframes"] * H * W * 4


def need_f64_planes(a):    # ... and for f64 frames the plane of low words next to it (+ 32 bytes)
    W, H, N, D = _geo(GENERIC)
    return a["nframes"] * H * W * 4 + 32


def need_cap_mm(a):        # fdoct_capture.cpp: 2 * nframes * blocks doubles; a frame of 64 runs wants one workgroup
    import stage_grid_sizes as sg
    runs = SIDE["H"] * -(-SIDE["W"] // sg.CAPTURE_RUN["u16"])
    return 2 * a["nframes"] * sg.minmax_blocks(runs, a["nframes"], 64) * 8


def need_col_sum(a):       # fdoct_route.cpp, run_colour: the sum frames, 16-byte-pitched rows of doubles
    return _pitch16(SIDE["W"] * 8) * SIDE["H"] * a["nframes"]


Growth = collections.namedtuple("Growth", "workspace site small large need")
GROWTH = [
    Growth("ws_ylin", "staged mode's k-linear rows", dict(nframes=1), dict(nframes=2), need_ylin),
    Growth("ws_cx", "process_complex_device, D x H", dict(nframes=1), dict(nframes=2), need_cx),
    Growth("ws_dop_bulk", "doppler_device with bulk", dict(nframes=1), dict(nframes=3), need_dop_bulk),
    Growth("ws_sim", "the sim variant's gather, averages 2", dict(nframes=2), dict(nframes=4), need_sim),
    Growth("ws_front", "set_frontend(0, 2, 2)", dict(nframes=1), dict(nframes=2), need_front),
    Growth("ws_med", "set_frontend(3, 1, 1)", dict(nframes=1), dict(nframes=2), need_med),
    Growth("ws_tr", "D x H through the transpose pass", dict(nframes=1), dict(nframes=2), need_tr),
    Growth("d_minmax", "whole-frame normalisation", dict(nframes=1), dict(nframes=2), need_minmax),
    Growth("ws_big_*", "the long-row path's chunk", dict(nframes=1), dict(nframes=2), need_big_y),
    Growth("d_sf_part", "saveframes_device with pictures", dict(nframes=1), dict(nframes=3), need_sf_part),
    Growth("ws_lp_bins", "lowpass_rows_device, rows of 5850", dict(rows=1), dict(rows=2), need_lp_bins),
    Growth("ws_cal_mm", "normalize_rows_minmax_device, per row", dict(rows=2), dict(rows=8), need_cal_mm),
    Growth("d_disp_part", "display_device", dict(nbscans=1), dict(nbscans=3), need_disp_part),
    Growth("ws_mov", "movavgn 3 on u16 frames", dict(nframes=1), dict(nframes=2), need_mov),
    Growth("ws_f32 + ws_f32_lo", "f64 frames, the split planes", dict(nframes=1), dict(nframes=2), need_f64_planes),
    Growth("ws_cap_mm", "frame_minmax_device", dict(nframes=1), dict(nframes=3), need_cap_mm),
    Growth("ws_col_sum", "colour_extract_device, channel 3", dict(nframes=1), dict(nframes=2), need_col_sum),
]
GROWTH_IDS = [g.workspace for g in GROWTH]
# handle-owned buffers that no pair can grow under a call in flight, and why
GROWTH_EXEMPT = {
    "ws_cap_acc": "H x W doubles of the handle's own geometry: the size never changes; every call that uses it returns drained",
    "ws_cal_next": "likewise H x W doubles, and swapped with its slot only after the capture has synchronised",
    "stage_in / stage_out": "used by calls with a host-memory argument only, and those return drained before the next call can grow them",
    "pl_* / pin_*": "the pipeline of the synchronous fdoct_process, which returns drained",
    "d_hold_cols": "replaced by set_peakhold_roi: the setter case of that name",
    "d_mavg": "replaced by manualavg_begin: the setter case of that name",
    "d_bin_taps": "re-uploaded by bscan_bin_device with a new factor: the setter case of that name",
    "ws_col": "the colour stage's median input: grows like ws_med behind it, on the same reserve path (run_colour, run_frontend)",
}
