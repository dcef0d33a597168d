"""The catalogue of tests/test_gpu_stream_order.py as plain Python: which Reconstructor methods enqueue on device memory (ENTRIES),
which change a handle's state (SETTERS), which public methods of either name pattern are left out and why (EXEMPT), and the pairs of
calls of which the second outgrows a handle-owned workspace the first is still using (GROWTH), with the workspace's size restated from
its `.reserve(` site.  tests/test_stream_cases.py holds the catalogue to fdoct_amd.capi.Reconstructor on the CPU -- a new `*_device`
or `set_*` method fails there until it is listed -- and every pair to "the second call needs strictly more bytes"; the GPU tests run
one case per name and fail on a name without a case.

The add-on stages (dispersion search, vibrometry, angiography, coherent averaging, SSADA) are module-level functions over a
Reconstructor: ADDON_ENTRIES names their ten `*_device` functions, ADDON_GROWTH the pairs of their workspaces (and of stage_out as
the scratch of a device-memory call), TABLE_PAIRS per stage two parameter sets that rewrite a handle-owned table of the same size.
tests/test_stream_cases.py walks the package's modules for such functions and holds the restated sizes to the stages' `*_plan`
entry points; tests/test_gpu_stream_order_stages.py runs the cases.

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
    "stage_in / stage_out for host memory": "a call with a host-memory argument returns drained before the next call can grow them; stage_in holds "
                                            "nothing else, and stage_out as scratch of a device-memory call is the pair 'stage_out (scratch)' of ADDON_GROWTH",
    "pl_* / pin_*": "the pipeline of the synchronous fdoct_process, which returns drained",
    "d_hold_cols": "replaced by set_peakhold_roi: the setter case of that name",
    "d_mavg": "replaced by manualavg_begin: the setter case of that name",
    "d_bin_taps": "re-uploaded by bscan_bin_device with a new factor: the setter case of that name",
    "ws_col": "the colour stage's median input: grows like ws_med behind it, on the same reserve path (run_colour, run_frontend)",
}


# ---- the add-on stages ------------------------------------------------------------------------------------------------------------------
# Module-level functions over a Reconstructor (fdoct_amd/dispersion.py, vibrometry.py, angiography.py, coherent.py, ssada.py), which
# must_be_listed() above does not see: tests/test_stream_cases.py walks the package's modules for them, and
# tests/test_gpu_stream_order_stages.py runs a case per name.
ADDON_ENTRIES = [
    "dispersion.search_device", "dispersion.process_search_device", "vibrometry.vibro_device", "vibrometry.process_vibro_device",
    "angiography.angio_device", "angiography.process_angio_device", "coherent.cxavg_device", "coherent.process_cxavg_device",
    "ssada.ssada_device", "ssada.process_ssada_device",
]
ADDON_EXEMPT = {}     # "module.function" -> why a module-level *_device function has no case
ADDON_STAGES = ["ssada", "dispersion", "vibro", "angio", "cxavg"]
FAR = 1e-3            # "far more than a bit" (tests/test_gpu_stream_order.py): a relative distance of 1e-3 is 2^14 float ulps


def addon_functions():
    """"module.function" of every module-level function of the fdoct_amd package whose name ends in _device."""
    import importlib
    import inspect
    import pkgutil

    import fdoct_amd
    found = []
    for info in pkgutil.iter_modules(fdoct_amd.__path__):
        spec = info.module_finder.find_spec("fdoct_amd." + info.name)
        if not (spec and spec.origin and spec.origin.endswith(".py")):
            continue          # the shared libraries next to the modules are no Python modules
        mod = importlib.import_module("fdoct_amd." + info.name)
        for name, f in vars(mod).items():
            if inspect.isfunction(f) and f.__module__ == mod.__name__ and name.endswith("_device"):
                found.append("%s.%s" % (info.name, name))
    return sorted(found)


def distance(a, b):
    """The largest elementwise |a - b| / max(|a|, |b|) over the common prefix of two outputs (0: the same values); a complex output
    counts as its (re, im) floats."""
    import numpy as np

    def floats(v):
        v = np.ascontiguousarray(v)
        if np.iscomplexobj(v):
            v = v.view(np.float64 if v.dtype == np.complex128 else np.float32)
        return v.reshape(-1).astype(np.float64)
    a, b = floats(a), floats(b)
    n = min(a.size, b.size)
    a, b = a[:n], b[:n]
    ok = np.isfinite(a) & np.isfinite(b)
    d = np.abs(a - b)[ok] / np.maximum(np.maximum(np.abs(a), np.abs(b))[ok], 1e-300)
    return float(d.max()) if d.size else 0.0


# A call of a stage is (shape, p): the input's shape and the keywords of the stage's model, which (but for dispersion's) are those of
# the binding's params() too.  Dispersion's p holds each axis as (first, step) and the counts as grid = (a2_count, a3_count).
def _align256(n_bytes):
    return (n_bytes + 255) & ~255             # StagePlan::kAlign (fdoct_stage.h)


def disp_axes(p):
    """(a2, a3, depth) as fdoct_amd.dispersion takes them."""
    return p["a2"] + (p["grid"][0],), p["a3"] + (p["grid"][1],), p.get("depth", (0, 0))


def ssada_bytes(shape, p):
    """fdoct_ssada_kernels.h: ssada_tab_bytes -- n twiddles (float2) and bands x n floats; fdoct_ssada.cpp, plan_ssada and run_stage:
    without a device out_bands, groups_per_pass shares of the band pairs, d and p (all groups: the default cap is 2 GiB)."""
    import ssada_cases
    import ssada_model
    n, M = shape["n"], p["bands"]
    dc = ssada_model.resolve(n, M, 1.0, (0, 0), p.get("depth", (0, 0)))[4]
    share = ssada_cases.group_share(p["repeats"], M, shape["ascans"], dc)
    cap = p.get("max_workspace_bytes", 0) or ssada_cases.DEFAULT_WORKSPACE
    return {"ws_ssa_tab": n * 8 + M * n * 4, "ws_ssa": min(shape["groups"], cap // share) * share}


def dispersion_bytes(shape, p, want=("sums", "row_sums", "best", "cos_sin")):
    """fdoct_dispersion_kernels.h: dispersion_tab_entries float2s; fdoct_dispersion.cpp, run_search with fdoct_stage.h's
    out_or_scratch: a null sums, row_sums or best of a device-memory call lies in stage_out, each from a multiple of 256 bytes."""
    n, rows, (c2, c3) = shape["n"], shape["rows"], p["grid"]
    K = c2 * c3
    out = {"sums": K * 16, "row_sums": rows * K * 16, "best": 40, "cos_sin": n * 8}
    scratch = sum(_align256(out[w]) for w in ("sums", "row_sums", "best") if w not in want)
    return {"ws_disp_tab": (1 + c2 + c3) * n * 8, "stage_out (scratch)": scratch, "outputs": sum(out.values())}


def vibro_bytes(shape, p, want=("amp", "rms", "drift", "power")):
    """fdoct_vibro.cpp, plan_vibro and drop_unread: the reference phasors, one float2 per frame and A-scan; the lock-in's double2
    tables (nfreq x T, 2 per chunk and slot, 3 per slot; slots = nfreq + 1); with more than one chunk 5 + 2 nfreq doubles per chunk
    and pixel.  Without amp the lock-in is dropped."""
    import vibro_model
    T, H, D = shape["nframes"], shape["ascans"], shape["depths"]
    nfreq = len(p.get("freq", ())) if "amp" in want else 0
    cs = min(p.get("chunk_steps", 0) or vibro_model.chunk_rule(T, H * D), T - 1)
    chunks = -(-(T - 1) // cs)
    slots = nfreq + 1
    return {"ws_vib_ref": T * H * 8 if p.get("ref") else 0,
            "ws_vib_tab": (nfreq * T + chunks * slots * 2 + 3 * slots) * 16 if nfreq else 0,
            "ws_vib_part": chunks * (5 + 2 * nfreq) * H * D * 8 if chunks > 1 else 0}


def angio_bytes(shape, p, want=("var", "decorr", "cdecorr", "power")):
    """fdoct_angio.cpp, plan_angio and drop_unread: one float2 per group, pair of repeats and A-scan, with bulk on and cdecorr asked for."""
    groups = shape["nframes"] // p["repeats"]
    return {"ws_ang_bulk": groups * (p["repeats"] - 1) * shape["ascans"] * 8 if p.get("bulk") and "cdecorr" in want else 0}


def cxavg_bytes(shape, p):
    """fdoct_cxavg.cpp, plan_cxavg: with align 2 a float2 phasor per group and repeat, and behind them one per group, repeat and A-scan."""
    R = p["repeats"]
    groups = (shape["nframes"] - R) // (p.get("stride") or R) + 1
    return {"ws_cxa": (groups * R + groups * R * shape["ascans"]) * 8 if p.get("align", 1) == 2 else 0}


STAGE_BYTES = {"ssada": ssada_bytes, "dispersion": dispersion_bytes, "vibro": vibro_bytes, "angio": angio_bytes, "cxavg": cxavg_bytes}


def addon_field(stage, shape, seed):
    """The input of a call: complex64, from the stage's own generator (tests/*_cases.py)."""
    import numpy as np
    if stage == "dispersion":
        import dispersion_cases
        return dispersion_cases.field(shape["n"], shape["rows"], (8.0, -2.0), seed)
    if stage == "vibro":
        import vibro_cases
        return vibro_cases.field(shape["nframes"], shape["ascans"], shape["depths"], seed, common=0.4, surface=(0, 1))
    import angio_cases
    if stage == "ssada":
        return angio_cases.field(shape["groups"], shape["repeats"], shape["ascans"], shape["n"], seed, kind="vessel")
    repeats = shape["repeats"]
    return angio_cases.field(shape["nframes"] // repeats, repeats, shape["ascans"], shape["depths"], seed, kind="vessel" if stage == "angio" else "static",
                             bulk_phase=1.0 if stage == "angio" else np.pi)


def addon_model(stage, X, p, truth=False):
    """The stage's NumPy model of a call, as the dict the model returns."""
    if stage == "ssada":
        import ssada_model
        return ssada_model.model(X, truth=truth, **p)
    if stage == "dispersion":
        import dispersion_model
        a2, a3, depth = disp_axes(p)
        return dispersion_model.model(X, a2, a3, depth, truth=truth)
    if stage == "vibro":
        import vibro_model
        return vibro_model.model(X, truth=truth, **p)
    if stage == "angio":
        import angio_model
        return angio_model.model(X, truth=truth, **p)
    import cxavg_model
    return cxavg_model.model(X, truth=truth, **p)


# ---- pairs of parameter sets that share a table -----------------------------------------------------------------------------------------
# Per stage one input shape and two parameter sets under which every handle-owned table of the call has the same size -- nothing is
# reserved anew and nothing drains between call A (p1) and call B (p2) -- and other contents.  `tables`: the workspaces the calls
# write per call; `main`: the output whose distance between "A under p1" and "A under p2" shows a reach-back.
TablePair = collections.namedtuple("TablePair", "stage shape p1 p2 tables main seed")
TABLE_PAIRS = [
    TablePair("ssada", dict(groups=1, repeats=2, ascans=3, n=60), dict(repeats=2, bands=3, sigma=10.0, win=(1, 1)),
              dict(repeats=2, bands=3, sigma=3.0, support=(6, 48), win=(1, 1)), ("ws_ssa_tab", "ws_ssa"), "decorr", 201),
    TablePair("dispersion", dict(rows=2, n=16), dict(a2=(-8.0, 8.0), a3=(0.0, 2.0), grid=(3, 1)), dict(a2=(-20.0, 4.0), a3=(-2.0, 2.0), grid=(3, 1)),
              ("ws_disp_tab",), "sums", 202),
    TablePair("vibro", dict(nframes=6, ascans=3, depths=5), dict(freq=(0.11,), ref=(0, 1)), dict(freq=(0.25,), ref=(4, 1)),
              ("ws_vib_ref", "ws_vib_tab"), "amp", 203),
    TablePair("angio", dict(nframes=4, repeats=2, ascans=3, depths=16), dict(repeats=2, win=(1, 1), bulk=(0, 8)), dict(repeats=2, win=(1, 1), bulk=(8, 8)),
              ("ws_ang_bulk",), "cdecorr", 204),
    TablePair("cxavg", dict(nframes=4, repeats=2, ascans=3, depths=16), dict(repeats=2, ref=0, align=2, align_range=(0, 8)),
              dict(repeats=2, ref=1, align=2, align_range=(8, 8)), ("ws_cxa",), "mean", 205),
]
TABLE_PAIR_IDS = [t.stage for t in TABLE_PAIRS]


# ---- growth pairs of the add-on stages ------------------------------------------------------------------------------------------------------
# As GROWTH above; a list of its own, because tests/test_gpu_stream_order.py holds its cases to GROWTH name by name.  `call`: (stage,
# shape, p, the outputs asked for) of call A; `small` and `large` name the one key of shape or p in which call B differs.
AddonGrowth = collections.namedtuple("AddonGrowth", "workspace site small large need call")


def addon_call(g, which):
    """(stage, shape, p, want) of call A (which = g.small) or call B (g.large)."""
    stage, shape, p, want = g.call
    shape, p = dict(shape), dict(p)
    for k, v in which.items():
        (shape if k in shape else p)[k] = v
    return stage, shape, p, want


def _addon_need(workspace):
    def need(g, which):
        stage, shape, p, want = addon_call(g, which)
        fn = STAGE_BYTES[stage]
        return (fn(shape, p) if stage in ("ssada", "cxavg") else fn(shape, p, want))[workspace]
    return need


_SSA = ("ssada", dict(groups=1, repeats=2, ascans=3, n=60), dict(repeats=2, bands=3, win=(1, 1)), ("decorr", "band_decorr", "power"))
_DISP = ("dispersion", dict(rows=2, n=16), dict(a2=(-8.0, 8.0), a3=(0.0, 2.0), grid=(3, 1)), ("sums", "row_sums", "best", "cos_sin"))
_VIB = ("vibro", dict(nframes=4, ascans=3, depths=5), dict(freq=(0.11,)), ("amp", "rms", "drift", "power"))
_ANG = ("angio", dict(nframes=2, repeats=2, ascans=3, depths=16), dict(repeats=2, win=(1, 1), bulk=(0, 8)), ("var", "decorr", "cdecorr", "power"))
_CXA = ("cxavg", dict(nframes=2, repeats=2, ascans=3, depths=16), dict(repeats=2, ref=0, align=2, align_range=(0, 8)), ("mean", "mag", "incoh", "coh"))
ADDON_GROWTH = [
    AddonGrowth("ws_ssa_tab", "ssada_tab_bytes: more bands", dict(bands=2), dict(bands=5), _addon_need("ws_ssa_tab"), _SSA),
    AddonGrowth("ws_ssa", "fdoct_ssada.cpp: more groups, no device out_bands", dict(groups=1), dict(groups=3), _addon_need("ws_ssa"), _SSA),
    AddonGrowth("ws_disp_tab", "dispersion_tab_entries: a larger grid", dict(grid=(3, 1)), dict(grid=(5, 2)), _addon_need("ws_disp_tab"), _DISP),
    AddonGrowth("ws_vib_ref", "fdoct_vibro.cpp, plan_vibro: more frames with a reference", dict(nframes=4), dict(nframes=8), _addon_need("ws_vib_ref"),
                _VIB[:2] + (dict(freq=(0.11,), ref=(0, 1)),) + _VIB[3:]),
    AddonGrowth("ws_vib_tab", "fdoct_vibro.cpp, plan_vibro: a second frequency", dict(freq=(0.11,)), dict(freq=(0.11, 0.25)), _addon_need("ws_vib_tab"), _VIB),
    AddonGrowth("ws_vib_part", "fdoct_vibro.cpp, plan_vibro: chunks of 2 steps, more frames", dict(nframes=4), dict(nframes=8), _addon_need("ws_vib_part"),
                _VIB[:2] + (dict(freq=(0.11,), chunk_steps=2),) + _VIB[3:]),
    AddonGrowth("ws_ang_bulk", "fdoct_angio.cpp: more groups, bulk on and cdecorr asked for", dict(nframes=2), dict(nframes=6), _addon_need("ws_ang_bulk"), _ANG),
    AddonGrowth("ws_cxa", "fdoct_cxavg.cpp: more groups under align 2", dict(nframes=2), dict(nframes=6), _addon_need("ws_cxa"), _CXA),
    AddonGrowth("stage_out (scratch)", "fdoct_stage.h, out_or_scratch: search_device that asks for cos_sin only, more rows", dict(rows=2), dict(rows=6),
                _addon_need("stage_out (scratch)"), _DISP[:3] + (("cos_sin",),)),
]
ADDON_GROWTH_IDS = [g.workspace for g in ADDON_GROWTH]
