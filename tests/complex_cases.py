"""The cases tests/test_gpu_complex_options.py puts through the two kernel forms that write the complex A-scan (the wave-per-row
kernel compiled at run time with FDOCT_WAVE_OPT_CXOUT, generic_kernel's CX form), as plain numpy: every chain option that selects
another kernel or another pass in front of it, rows with a phase displayed beyond numfftpoints / 2, depths off the 64-bin grid,
the degenerate frames and planes of tests/degenerate_cases.py and the caller-supplied tables of tests/resample_tables.py.
tests/test_complex_cases.py holds every case to its conditions on the CPU, with the reference alone.

Option, phase and depth cases are 2 frames of 12 rows; the degenerate and the table cases keep their own 11-row frame.

One (family, table) pair is left out, DROPPED_PAIRS: under `evenodd` on the 161 x 4 full-length zero-pad the float composition is
itself 0.364 x the tolerance from the composition in double, beyond resample_tables.ORACLE_LIMIT = 0.25 -- there the reference, not
the kernel, would set what the GPU is allowed.  Every other pair of the eight families holds it."""
import collections
import functools

import numpy as np

import degenerate_cases as dg
import resample_tables as rt
from fdoct_amd import VARIANT_SIM, Config, synth

H, NF = 12, 2
FIRST_FRAME = 4                       # synth.make_frames' first frame number
WAVE_SHAPE = (200, 4, 2560, 320)      # (W, M, N, D)
GENERIC_SHAPE = (2048, 1, 2002, 1001)
GENERIC_BANDPASS_SHAPE = (322, 4, 1288, 320)   # the band-pass lives in the zero-pad stage: M > 1
EDGE_SHAPE = (640, 1, 640)            # (W, M, N) of the phase and depth cases
MOVAVGN = 3

# what process_complex takes, what the model takes (data_y after the front end), and the keywords of complex_model.model and of
# the handle (yp, yd, phase, window, bandpass; the handle's also: frontend, colour, jit)
Setup = collections.namedtuple("Setup", "cfg frames model_frames yb mkw hkw")


def shape_name(W, M, N, D):
    return ("%d x%d -> %d, D %d" % (W, M, N, D)) if M > 1 else ("%d -> %d, D %d" % (W, N, D))


def hamming(W):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1))


def _non_integer(frames, rng, dtype):
    """Sample values no integer type holds: a seventh of the counts plus noise below one count."""
    f = (frames.astype(np.float64) / 7.0 + rng.uniform(-0.5, 0.5, frames.shape)).astype(dtype)
    f[f == np.rint(f)] += 0.25          # (a float of a few thousand counts has steps of 2^-11: some land on a whole count)
    assert not np.any(f == np.rint(f))
    return f


# ---- a. options --------------------------------------------------------------------------------------------------------------------
# kind: the option; route: 'wave' | 'generic', the kernel form the SHAPE reaches; family: the form the case runs.  They differ
# where the pass in front of the chain hands the samples over as two float planes, a high and a low word -- doubles
# (PrePass::F64Split, MovAvgF64: f64 frames, the colour sum) and the tap sums of non-integer floats (MovAvgF32Wide): the
# wave-per-row kernel does not take the low plane (fdoct_route_value.cpp: wave_scope), so on its shape those cases run generic_kernel
# on the zero-padded 200 x 4 row, a third geometry of the CX form.
Option = collections.namedtuple("Option", "name route family shape kind")
LOW_WORD_KINDS = ("movavgn 3, f32 non-integer frames", "movavgn 3, f64 non-integer frames", "colour handle, channel 3")
KINDS = ("band-pass", "rowwisenormalize", "whole-frame normalise", "movavgn 3, u16 frames", "movavgn 3, f32 non-integer frames",
         "movavgn 3, f64 non-integer frames", "full-frame background", "Hamming window", "f32 frames", "median 3 of raw u8 frames",
         "colour handle, channel 1", "colour handle, channel 3")
FOUR_BITS = "band-pass + rowwisenormalize + pi + dark"


def _option(route, kind):
    shape = WAVE_SHAPE if route == "wave" else GENERIC_BANDPASS_SHAPE if kind == "band-pass" else GENERIC_SHAPE
    family = "generic" if kind in LOW_WORD_KINDS else route
    return Option("%s: %s, %s" % (family, shape_name(*shape), kind), route, family, shape, kind)


OPTION_CASES = [_option("wave", k) for k in KINDS + (FOUR_BITS,)] + [_option("generic", k) for k in KINDS]


@functools.lru_cache(maxsize=None)
def option_setup(case):
    W, M, N, D = case.shape
    kind = case.kind
    rng = np.random.default_rng(31)
    ckw, mkw, hkw = {}, {}, {}
    frames = synth.make_frames(FIRST_FRAME, NF, W, H)
    model_frames = frames
    yb = synth.make_background(W).astype(np.float64)
    if kind in ("band-pass", FOUR_BITS):
        assert M > 1
        mkw["bandpass"], hkw["bandpass"] = 1, True
    if kind in ("rowwisenormalize", FOUR_BITS):
        ckw["rowwisenormalize"] = 1
        yb = yb / 65535.0                       # (the normalisations leave samples in [0, 1])
    if kind == FOUR_BITS:
        mkw["yp"] = hkw["yp"] = rng.uniform(0.0, 0.02, (H, W))
        mkw["yd"] = hkw["yd"] = rng.uniform(90.0, 110.0, (H, W))
    if kind == "whole-frame normalise":
        ckw["donotnormalize"] = 0
        yb = yb / 65535.0
    if kind.startswith("movavgn"):
        ckw["movavgn"] = MOVAVGN
    if "non-integer" in kind or kind == "f32 frames":
        frames = model_frames = _non_integer(frames, rng, np.float64 if "f64" in kind else np.float32)
        yb = yb / 7.0
    if kind == "full-frame background":
        yb = np.clip(np.rint(yb[None, :] * (0.8 + 0.4 * rng.random((H, 1)))), 1.0, 65535.0)
    if kind == "Hamming window":
        mkw["window"] = hkw["window"] = hamming(W)
    if kind.startswith("median"):
        import oracle_lib as orc
        frames = synth.make_frames(FIRST_FRAME, NF, W, H, dtype=np.uint8)
        model_frames = np.stack([orc.median_blur(f, 3) for f in frames])       # cv::medianBlur as the oracle states it
        yb = synth.make_background(W, dtype=np.uint8).astype(np.float64)
        hkw["frontend"] = (3, 1, 1)
    if kind.startswith("colour"):
        import colour_model
        c = int(kind[-1])
        frames = np.stack([synth.make_frames(FIRST_FRAME + 5 * ch, NF, W, H, dtype=np.uint8) for ch in range(3)], axis=-1)
        model_frames = colour_model.extract(frames, c)                         # what the colour stage leaves: u8, or doubles (3)
        yb = synth.make_background(W, dtype=np.uint8).astype(np.float64)
        if c == 3:
            yb = 3.0 * yb * colour_model.SUM_SCALE
        hkw["colour"] = c
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, **ckw)
    for a in (frames, model_frames, yb):
        a.setflags(write=False)
    return Setup(cfg, frames, model_frames, yb, mkw, hkw)


# ---- b. phase beyond numfftpoints / 2, c. depth edges ---------------------------------------------------------------------------------
# route 'generic': the same shape with run-time compilation off
Edge = collections.namedtuple("Edge", "name route D phase")
PHASE_DEPTHS = (640, 641 - 300)
DEPTHS = (1, 63, 64, 65, 320, 321, 640)        # 321 = N / 2 + 1: bin N / 2 alone lies beyond the half; 640 = N


def _edge(route, D, note, phase=False):
    return Edge("%s: %s, %s" % (route, shape_name(EDGE_SHAPE[0], 1, EDGE_SHAPE[2], D), note), route, D, phase)


PHASE_CASES = [_edge(r, D, "dispersion phase" if p else "no phase (the mirror control)", p) for r in ("wave", "generic") for p in (True, False)
               for D in PHASE_DEPTHS]
DEPTH_CASES = [_edge(r, D, "depth edge") for r in ("wave", "generic") for D in DEPTHS]


@functools.lru_cache(maxsize=None)
def edge_setup(case):
    W, M, N = EDGE_SHAPE
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=case.D, increasefftpointsmultiplier=M)
    frames = synth.make_frames(FIRST_FRAME, NF, W, H)
    yb = synth.make_background(W).astype(np.float64)
    mkw, hkw = {}, {}
    if case.phase:
        mkw["phase"] = hkw["phase"] = synth.dispersion_phase(N)
    if case.route == "generic":
        hkw["jit"] = False
    for a in (frames, yb):
        a.setflags(write=False)
    return Setup(cfg, frames, frames, yb, mkw, hkw)


# ---- d. degenerate rows --------------------------------------------------------------------------------------------------------------
DEGENERATE_FAMILIES = ("wave-per-row, run-time compiled, 200 x 4", "workgroup-per-row, 2048 -> 2002")
DEGENERATE_CASES = [dg.C("plain", "clean"), dg.C("plain", "dead"), dg.C("plain", "full"), dg.C("rowwise", "full"), dg.C("whole", "dead"),
                    dg.C("sim", "clean"), dg.C("plain", "dead", extra="pi"), dg.C("plain", "dead", extra="dark"),
                    dg.C("whole", "clean", "constant"), dg.C("whole", "clean", "corners")]       # (no pair: averages must be 1)
ISOLATION_CASES = [dg.C("plain", "dead"), dg.C("rowwise", "dead")]


def degenerate_name(fam_name, case):
    return "%s, %s/%s%s%s" % (fam_name, case.opt, case.bg, "" if case.frames == "one" else "/" + case.frames, " + " + case.extra if case.extra else "")


def degenerate_rows(case):
    """(empty, cancelled) of complex_model.check_rows: the rows that are empty only because a DC level cancels (the no-fringe row,
    the constant rows under row-wise normalisation) are `cancelled`, every other exactly empty row is `empty`."""
    cancelled = dg.dc_level_rows(case)
    return [r for r in dg.exact_empty_rows(case) if r not in cancelled], cancelled


def copy_is_exact(case):
    """Row 10 repeats row 0 and must give its bits: a one-row background and no whole-frame normalisation."""
    return case.bg != "full" and case.opt in ("plain", "rowwise") and case.frames == "one"


def degenerate_mkw(i):
    return {k: v for k, v in (("yp", i.yp), ("yd", i.yd)) if v is not None}


# ---- e. caller tables ----------------------------------------------------------------------------------------------------------------
TABLE_FAMILIES = ("wave-per-row, run-time compiled, 200 x 4", "wave-per-row, complex rows, 160 x 4", "wave-per-row, 1280 x 4 -> 2560",
                  "wave-per-row, 640 x 4, tables in registers", "workgroup-per-row, 2048 -> 2002",
                  "workgroup-per-row, complex rows, 2048 -> 2002", "workgroup-per-row, full-length zero-pad, 161 x 4",
                  "workgroup-per-row, Bluestein, 322 x 4")
# the float composition alone is 0.364 x the tolerance from the composition in double: beyond resample_tables.ORACLE_LIMIT
DROPPED_PAIRS = [("workgroup-per-row, full-length zero-pad, 161 x 4", "evenodd")]
TABLE_EMPTY, TABLE_CANCELLED = [dg.ZEROS], [dg.NO_FRINGE]     # resample_tables.CASE is plain / clean


def wave_family(fam_name):
    """Whether the complex call runs the family on the wave-per-row kernel (always the run-time compiled one)."""
    return fam_name.startswith("wave-per-row")


def tables_of(fam_name):
    return [t for t in rt.family(fam_name).tables if (fam_name, t) not in DROPPED_PAIRS]


def table_mkw(fam_name, t):
    i = rt.inputs(fam_name)
    kw = dict(table=rt.family_table(fam_name, t))
    if i.phase is not None:
        kw["phase"] = i.phase
    if rt.window(t, i.cfg.width) is not None:
        kw["window"] = rt.window(t, i.cfg.width)
    return kw


# ---- the reference, computed once and shared ----------------------------------------------------------------------------------------
def _models(cfg, frames, yb, mkw):
    import complex_model as cm
    ref, truth = cm.model(cfg, frames, yb, **mkw), cm.model(cfg, frames, yb, truth=1, **mkw)
    ref.setflags(write=False)
    truth.setflags(write=False)
    return ref, truth


@functools.lru_cache(maxsize=None)
def setup_models(case):
    """(float composition, composition in double) of an option, phase or depth case."""
    s = option_setup(case) if isinstance(case, Option) else edge_setup(case)
    return _models(s.cfg, s.model_frames, s.yb, s.mkw)


@functools.lru_cache(maxsize=None)
def degenerate_models(fam_name, case):
    i = dg.inputs(fam_name, case)
    return _models(i.cfg, i.frames, i.yb, degenerate_mkw(i))


@functools.lru_cache(maxsize=None)
def table_models(fam_name, t):
    i = rt.inputs(fam_name)
    return _models(i.cfg, i.frames, i.yb, table_mkw(fam_name, t))


def eps_chain(cfg):
    return 1e-6 if cfg.variant == VARIANT_SIM else 1e-5
