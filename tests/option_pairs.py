"""The options of the reconstruction chain laid over every kernel family as a covering array, as plain numpy: per family a list of
cases such that EVERY pair of levels of two different options that some admissible case can hold together is held by at least one
case.  tests/test_option_pairs.py proves that property by brute force over the constraint predicates, independently of the
generator, and holds every case to its conditions on the CPU (admissible, the expected kernel the one make_route decides, the f32
restatement within resample_tables.ORACLE_LIMIT of the chain in double); tests/test_gpu_option_pairs.py runs the cases.

What the array is for: every family writes the options out again in its own code, and the fixed suites hold them to the oracle one
at a time.  A defect in a line that two options share -- the frame index of the whole-frame extremes under averaging, the low
word's residuals scaled by a normalisation, the D x H store next to a null output -- is wrong only when both are on.

The options (FACTORS; a family declares the levels it has, the first level of an option it does not declare is what it runs with):

  samples     u8 | u16 | f32 (integer-valued) | f64 (NON-integer doubles in every case: the reference of such a case is composed
              from orc.frame_to_mag, which takes doubles with every other option -- f64_integer() says so per case)
  background  row | frame (rows scaled 0.8 ... 1.2)
  pi, dark    none | row | frame (the dark frame integer-valued)
  norm        none | rowwise | whole (donotnormalize = 0) | sim (the sim variant: whole-frame, eps 1e-6, the group's last frame)
  averages    1 | 2 | 3, two groups per call; from the second frame of a group on at half range, so per-frame extremes differ
  movavgn     0 | 2
  phase       off | on (synth.dispersion_phase)
  display     crop (0.3 N rounded up to an odd number: off the 64-bin grid; 320 on the D x H store) | half (N / 2) | deep (0.73 N)
  layout      HxD | DxH
  outputs     both | bscan | db
  division    two | one (set_precise_division(False))
  entry       host | device (packed rows, aligned) | offgrid (device pointers: a padded pitch, the base 4 bytes off the 16-byte
              grid -- 8 bytes for doubles --, the outputs one float off it)
  front       none | bin2 (2 x 2 binning) | med3bin2 (median 3, then 2 x 2 binning); raw frames as fuzz_cases.py makes them
  bandpass    off | on
  launch      auto | grid2 (set_launch(0, 2))
  window      built | hamming"""
import collections
import functools
import itertools

import numpy as np

import degenerate_cases as dg
import resample_tables as rt
from fdoct_amd import VARIANT_MAIN, VARIANT_SIM, Config, capi, synth

FACTORS = collections.OrderedDict([
    ("samples", ("u16", "u8", "f32", "f64")),
    ("background", ("row", "frame")),
    ("pi", ("none", "row", "frame")),
    ("dark", ("none", "row", "frame")),
    ("norm", ("none", "rowwise", "whole", "sim")),
    ("averages", (1, 2, 3)),
    ("movavgn", (0, 2)),
    ("phase", ("off", "on")),
    ("display", ("half", "crop", "deep")),
    ("layout", ("HxD", "DxH")),
    ("outputs", ("both", "bscan", "db")),
    ("division", ("two", "one")),
    ("entry", ("host", "device", "offgrid")),
    ("front", ("none", "bin2", "med3bin2")),
    ("bandpass", ("off", "on")),
    ("launch", ("auto", "grid2")),
    ("window", ("built", "hamming")),
])
NAMES = tuple(FACTORS)
Case = collections.namedtuple("Case", NAMES + ("frame",))     # frame: synth's frame number of the case's first frame
DEFAULT = {f: lv[0] for f, lv in FACTORS.items()}
SYNTH_FRAME = 11
GROUPS = 2
ROWS = 5                 # odd: on the 512-point plan (four rows per wave) rows of different frames share a wave
SEED = 20261
TARGET = 32              # cases per family aimed at; coverage wins where a family needs more (none does: 11 ... 25)
CANDIDATES = 24

# ---- the families ------------------------------------------------------------------------------------------------------------------
# setup: None | 'any-option' | 'staged' | 'rows-in-hbm' | 'dxh-store' (the family of the chain's own D x H store: its cases are the
# combinations tro_configured compiles, everything else in that layout belongs to the fast-path family next to it)
Family = collections.namedtuple("Family", "name geometry H setup levels kernels")


def _levels(**kw):
    lv = collections.OrderedDict()
    for f in NAMES:
        if f in kw:
            assert set(kw[f]) <= set(FACTORS[f]), (f, kw[f])
            lv[f] = tuple(kw[f])
    assert set(kw) <= set(NAMES), set(kw) - set(NAMES)
    return lv


_ALL = {f: FACTORS[f] for f in NAMES}
_INT = ("u16", "u8")
_ALIGNED = ("host", "device")        # a base off the 16-byte grid on a fused plan runs generic_kernel: another family
_SHALLOW = ("half", "crop")          # beyond numfftpoints / 2 a geometry has no fused plan (fdoct_plan.cpp): another family's kernel runs
# the fast path: 8/16-bit samples, no pi or dark frame, no moving average (its output is a float plane), real rows
# (fdoct_launch.cpp, make_fused_launch: `lean`)
_FAST = _levels(samples=_INT, background=_ALL["background"], norm=_ALL["norm"], averages=_ALL["averages"], display=_SHALLOW,
                layout=_ALL["layout"], outputs=_ALL["outputs"], division=_ALL["division"], entry=_ALIGNED, front=_ALL["front"],
                launch=_ALL["launch"], window=_ALL["window"])
# the any-option kernel: everything a fused plan takes
_ANY = _levels(**{**_ALL, "display": _SHALLOW, "entry": _ALIGNED, "bandpass": ("off",)})
# staged mode: the plain 16-bit set-up (fdoct_launch.cpp:132, "staged mode is built for the plain u16 acquisition configuration only")
_STAGED = _levels(averages=_ALL["averages"], display=_SHALLOW, layout=_ALL["layout"], outputs=_ALL["outputs"], division=_ALL["division"],
                  entry=_ALIGNED, launch=_ALL["launch"], window=_ALL["window"])
# the D x H store (fdoct_launch.cpp:35-50, tro_configured; fdoct_route_value.cpp:60-70, transposed_store_callable): 8/16-bit frames
# as they are (no front end, no moving average), aligned, no pi or dark frame, no row-wise normalisation, depth bins in whole
# write-out steps; on the 1024-point plan a full-frame background and the whole-frame normalisation too (with one frame per B-scan:
# the predicate below), on the 512-point plan the plain and the averaging kernel only
_DXH_1024 = _levels(samples=_INT, background=_ALL["background"], norm=("none", "whole", "sim"), averages=_ALL["averages"], display=_SHALLOW,
                    layout=("DxH",), outputs=_ALL["outputs"], division=_ALL["division"], entry=_ALIGNED, launch=_ALL["launch"],
                    window=_ALL["window"])
_DXH_512 = _levels(samples=_INT, averages=_ALL["averages"], display=_SHALLOW, layout=("DxH",), outputs=_ALL["outputs"],
                   division=_ALL["division"], entry=_ALIGNED, launch=_ALL["launch"], window=_ALL["window"])
_ROWS_M1 = _levels(**{**_ALL, "bandpass": ("off",)})      # band-pass needs increasefftpointsmultiplier > 1 (fdoct_set_bandpass)
_ROWS = _levels(**_ALL)
# the 65536-point rows: the oracle takes a second per case there; the long-row path's full option set runs on 161 x 4
_LONG = _levels(background=_ALL["background"], dark=_ALL["dark"], norm=_ALL["norm"], averages=_ALL["averages"], layout=_ALL["layout"],
                window=_ALL["window"])

K = capi
_FUSED_SET = (K.KERNEL_FUSED,)
_WAVE_SET = (K.KERNEL_WAVE, K.KERNEL_WAVE_JIT, K.KERNEL_GENERIC)


def _family(name, levels, kernels, setup="inherit", H=ROWS):
    f = rt.family(name)
    return Family(name, f.geometry, H, f.setup if setup == "inherit" else setup, levels, kernels)


FAMILIES = [
    _family("fused fast path, 512-point plan", _FAST, _FUSED_SET),
    _family("fused fast path, 1024-point plan", _FAST, _FUSED_SET),
    _family("fused fast path, 2048-point plan", _FAST, _FUSED_SET),
    _family("fused fast path, D x H, 1024-point plan", _DXH_1024, (K.KERNEL_FUSED_TRANSPOSED,), setup="dxh-store", H=8),   # (the store takes rows in fours)
    _family("fused fast path, D x H, 512-point plan", _DXH_512, (K.KERNEL_FUSED_TRANSPOSED,), setup="dxh-store", H=8),
    _family("fused any-option kernel", _ANY, _FUSED_SET),
    _family("fused, staged", _STAGED, (K.KERNEL_FUSED_STAGED,)),
    _family("wave-per-row, 160 x 4", _ROWS, _WAVE_SET),
    _family("wave-per-row, 640 x 1, 8-bit", _ROWS_M1, _WAVE_SET),
    _family("wave-per-row, run-time compiled, 200 x 4", _ROWS, (K.KERNEL_WAVE_JIT, K.KERNEL_GENERIC)),
    _family("workgroup-per-row, 2048 -> 2002", _ROWS_M1, (K.KERNEL_GENERIC,)),
    _family("workgroup-per-row, Bluestein, 322 x 4", _ROWS, (K.KERNEL_GENERIC,)),
    _family("workgroup-per-row, 1024 threads, 2400 x 4", _ROWS, (K.KERNEL_GENERIC,)),
    _family("long rows, 2048 x 8", _LONG, (K.KERNEL_LONG_ROWS,), H=3),
    _family("rows in HBM, 161 x 4", _ROWS, (K.KERNEL_LONG_ROWS,)),
]
FAMILY_IDS = [f.name for f in FAMILIES]
assert set(dg.FAMILY_IDS) <= set(FAMILY_IDS)


def family(name):
    return FAMILIES[FAMILY_IDS.index(name)]


def shape(fam):
    g = fam.geometry
    return g["width"], g["increasefftpointsmultiplier"], g["numfftpoints"]


def display_points(fam, level):
    N = shape(fam)[2]
    if level == "half":
        return N // 2
    if level == "deep":
        return int(0.73 * N)
    if fam.setup == "dxh-store":
        return 320                       # whole write-out steps of 64 bins (fdoct_launch.cpp:43)
    return int(np.ceil(0.3 * N)) | 1     # odd: off every grid


def library_averages(case):
    """Frames per output B-scan as the kernels see them: the sim variant emits the last frame of every group, which the library
    gathers in front of the chain (fdoct_hostcall.h: SimFrames) -- its kernels run with A = 1."""
    return 1 if case.norm == "sim" else case.averages


# ---- the constraints ---------------------------------------------------------------------------------------------------------------
# scope: the options the predicate reads (tests/test_option_pairs.py hands it nothing else); where: the line it comes from
Constraint = collections.namedtuple("Constraint", "name scope pred where")
CONSTRAINTS = [
    Constraint("the front end takes the camera's 8- or 16-bit frames", ("front", "samples"),
               lambda fam, c: c["front"] == "none" or c["samples"] in _INT, "fdoct_route_value.cpp:165"),
    Constraint("band-pass needs a zero-pad multiplier above 1", ("bandpass",),
               lambda fam, c: c["bandpass"] == "off" or shape(fam)[1] > 1, "fdoct_capi.cpp: fdoct_set_bandpass"),
    Constraint("the D x H store with a full-frame background or the whole-frame normalisation: one frame per B-scan",
               ("background", "norm", "averages"),
               lambda fam, c: fam.setup != "dxh-store" or not (c["background"] == "frame" or c["norm"] in ("whole", "sim")) or
               c["norm"] == "sim" or c["averages"] == 1, "fdoct_launch.cpp:41"),
]


def admissible(fam, case):
    c = case._asdict() if isinstance(case, Case) else case
    return all(c[f] in fam.levels.get(f, (DEFAULT[f],)) for f in NAMES) and all(k.pred(fam, c) for k in CONSTRAINTS)


# ---- what last_kernel() must report --------------------------------------------------------------------------------------------------
def low_word_plane(case):
    """Frames that reach the chain as two float planes, hi + lo: doubles, and float frames through the moving average
    (fdoct_route_value.cpp:172-187).  The wave-per-row kernels do not take the second plane (wave_scope)."""
    return case.samples == "f64" or (case.samples == "f32" and case.movavgn > 0)


def wave_options(fam, case):
    """The wave-per-row kernel's compile-time options a case turns on (fdoct_route_value.cpp:116-119), by name."""
    W, M, N = shape(fam)
    on = []
    if case.pi != "none":
        on.append("pi")
    if case.dark != "none":
        on.append("dark")
    if case.bandpass == "on" and M > 1:
        on.append("bandpass")
    if case.norm == "rowwise":
        on.append("rownorm")
    elif case.norm != "none":
        on.append("framenorm")
    if case.phase == "on":
        on.append("cplx")
    elif display_points(fam, case.display) > N // 2:
        on.append("deep")
    return tuple(on)


def binned_in_kernel(fam, case):
    """2 x 2 binning with nothing else in front of the chain goes into the loads of the run-time compiled wave-per-row kernel
    (fdoct_route_value.cpp:145-158): 16-bit samples (8-bit ones on rows of at most 320), real rows, no deep display, no whole-frame
    normalisation, no moving average."""
    W, M, N = shape(fam)
    return (case.front == "bin2" and (case.samples == "u16" or (case.samples == "u8" and W <= 320)) and case.movavgn == 0 and
            case.phase == "off" and display_points(fam, case.display) <= N // 2 and case.norm in ("none", "rowwise"))


def kernel_samples(case):
    """The sample type the chain's kernel reads: floats behind the moving average and for doubles."""
    return "f32" if case.movavgn > 0 or case.samples == "f64" else case.samples


def compile_key(fam, case):
    """What a run-time compiled kernel is compiled for besides the geometry: sample type, display and option set -- None where the
    case runs no such kernel."""
    if expected_kernel(fam, case) != K.KERNEL_WAVE_JIT:
        return None
    return (kernel_samples(case), case.display, wave_options(fam, case) + (("bin2",) if binned_in_kernel(fam, case) else ()))


def expected_kernel(fam, case):
    """As degenerate_cases.expected_kernel: the family's own kernel, and for the wave-per-row shapes what fdoct_route_value.cpp
    makes of the options -- the built-in kernel with no option on, the run-time compiled one as soon as an option bit is set (or
    the kernel bins; complex rows run the whole N-point transform, so a display beyond N / 2 is no option of theirs),
    generic_kernel where a low-word plane is handed over."""
    if fam.setup == "staged":
        return K.KERNEL_FUSED_STAGED
    if fam.setup == "dxh-store":
        return K.KERNEL_FUSED_TRANSPOSED
    if K.KERNEL_WAVE_JIT not in fam.kernels:
        return fam.kernels[0]            # (D x H outside the store's set: KERNEL_FUSED and the transpose pass)
    if low_word_plane(case):
        return K.KERNEL_GENERIC
    if binned_in_kernel(fam, case):
        return K.KERNEL_WAVE_JIT
    opts = wave_options(fam, case)
    if not opts and K.KERNEL_WAVE in fam.kernels:
        return K.KERNEL_WAVE
    return K.KERNEL_WAVE_JIT


# ---- the array -----------------------------------------------------------------------------------------------------------------------
def pairs_of(case):
    c = case._asdict() if isinstance(case, Case) else case
    return {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(NAMES, 2)}


def _construct(fam, rng, forced, covered):
    """One candidate: the forced levels, then the other options in random order, each at the level that holds the most pairs not
    yet covered with the options already set (ties: at random) among those no constraint refuses.  None at a dead end."""
    c = dict(forced)
    order = [f for f in NAMES if f not in c]
    rng.shuffle(order)
    for f in order:
        best, best_gain = [], -1
        for lv in fam.levels.get(f, (DEFAULT[f],)):
            c[f] = lv
            if not all(k.pred(fam, c) for k in CONSTRAINTS if f in k.scope and all(s in c for s in k.scope)):
                continue
            gain = sum(1 for g in c if g != f and _pair(f, lv, g, c[g]) not in covered)
            if gain > best_gain:
                best, best_gain = [lv], gain
            elif gain == best_gain:
                best.append(lv)
        if not best:
            return None
        c[f] = best[int(rng.integers(len(best)))]
    return c if admissible(fam, c) else None


def _pair(f, lf, g, lg):
    return ((f, lf), (g, lg)) if NAMES.index(f) < NAMES.index(g) else ((g, lg), (f, lf))


@functools.lru_cache(maxsize=None)
def generate(fam_name, seed=SEED):
    """The family's cases, greedily, after its plain set-up: every round seeds CANDIDATES candidates with a pair not yet covered and keeps the one that
    covers the most new pairs -- among equals one that compiles no new kernel at run time (each option set of the run-time compiled
    kernel is a compile of several seconds).  A pair no candidate could be built around in 64 tries counts as not admissible; the
    brute force of tests/test_option_pairs.py checks that belief."""
    fam = family(fam_name)
    rng = np.random.default_rng([seed, FAMILY_IDS.index(fam_name)])
    levels = {f: fam.levels.get(f, (DEFAULT[f],)) for f in NAMES}
    todo = [_pair(a, la, b, lb) for a, b in itertools.combinations(NAMES, 2) for la in levels[a] for lb in levels[b]]
    covered, hopeless, cases, keys = set(), set(), [], set()
    # the family's plain set-up first: the one case that runs its kernel with every option off (the built-in wave-per-row kernel)
    plain = {f: levels[f][0] for f in NAMES}
    assert admissible(fam, plain)
    cases.append(Case(frame=SYNTH_FRAME + 100 * REDRAWN.get((fam_name, 0), 0), **plain))
    covered |= pairs_of(plain)
    while True:
        open_pairs = [p for p in todo if p not in covered and p not in hopeless]
        if not open_pairs:
            break
        cands = []
        for t in range(CANDIDATES):
            p = open_pairs[int(rng.integers(len(open_pairs)))] if t else open_pairs[0]
            c = _construct(fam, rng, dict(p), covered)
            if c is not None:
                cands.append(c)
        if not cands:
            # nothing could be built around any of the pairs tried: look at the first open pair alone, for longer
            p = open_pairs[0]
            for t in range(64):
                c = _construct(fam, rng, dict(p), covered)
                if c is not None:
                    cands.append(c)
                    break
            else:
                hopeless.add(p)
                continue
        def score(c):
            case = Case(frame=SYNTH_FRAME, **c)
            key = compile_key(fam, case)
            return (len(pairs_of(c) - covered), key is None or key in keys)
        best = max(cands, key=score)
        case = Case(frame=SYNTH_FRAME + 100 * REDRAWN.get((fam_name, len(cases)), 0), **best)
        cases.append(case)
        covered |= pairs_of(best)
        keys.add(compile_key(fam, case))
    return tuple(cases)


# (family, index of the case) -> how many times its frames were redrawn to hold the oracle condition (tests/test_option_pairs.py)
REDRAWN = {}
# family -> the admissible pairs no case within the oracle condition could be built around, with the f32 restatement's measured
# distance from the chain in double (at most 2 % of the family's admissible pairs; the CPU test holds the list to what the array misses)
UNCOVERED_PAIRS = {}


def row_independence_case(fam_name):
    """The family's first whole-frame-normalised case with averages > 1 -- the joint where normalisation, averaging and the frame
    index of the extremes meet; where the family has none (staged mode, the D x H store), its first case with averages > 1."""
    cases = generate(fam_name)
    for want in (lambda c: c.norm == "whole" and c.averages > 1, lambda c: c.averages > 1):
        for c in cases:
            if want(c):
                return c
    return None


def case_id(case):
    return "-".join(str(getattr(case, f)) for f in NAMES if getattr(case, f) != DEFAULT[f]) or "defaults"


# ---- the inputs of a case --------------------------------------------------------------------------------------------------------------
def f64_integer(case):
    """Whether a case's f64 samples are integer-valued: never -- the reference of an f64 case is composed from orc.frame_to_mag,
    which takes doubles together with every other option (as test_f64_frames_with_non_integer_samples does)."""
    return False


def config(fam, case):
    return Config(height=fam.H, numdisplaypoints=display_points(fam, case.display), averages=case.averages,
                  rowwisenormalize=int(case.norm == "rowwise"), donotnormalize=0 if case.norm == "whole" else 1, movavgn=case.movavgn,
                  variant=VARIANT_SIM if case.norm == "sim" else VARIANT_MAIN,
                  **{k: v for k, v in fam.geometry.items() if k != "numdisplaypoints"})


def hamming(W):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1))


Inputs = collections.namedtuple("Inputs", "cfg frames oracle_frames yb yp yd phase window bandpass front")


@functools.lru_cache(maxsize=64)
def inputs(fam_name, case):
    """cfg; frames as the handle takes them (raw camera frames behind a front end); oracle_frames as the reference takes them (the
    CPU-binned frames; doubles for f64 samples); the background, pi and dark frames; phasors, window (None: the built one), band-pass
    switch and the front end's (median, binx, biny) or None."""
    import oracle_lib as orc
    fam = family(fam_name)
    W, H = fam.geometry["width"], fam.H
    A = case.averages
    rng = np.random.default_rng([SEED, case.frame, A])
    frames = synth.make_frames(case.frame, GROUPS * A, max(W, 64), H)[:, :, :W].copy()
    for g in range(GROUPS):
        frames[g * A + 1:(g + 1) * A] >>= 1          # (a group's later frames at half range)
    yb = synth.make_background(max(W, 64))[:W].astype(np.float64) + 10.0
    if case.samples == "u8":
        frames = (frames >> 8).astype(np.uint8)
        yb = yb / 256.0 + 1.0
    if case.background == "frame":
        yb = yb[None, :] * (0.8 + 0.4 * rng.random((H, 1)))
    top = float(frames.max())
    shp = {"row": (W,), "frame": (H, W)}
    yp = 0.01 * top * rng.random(shp[case.pi]) if case.pi != "none" else None
    yd = np.rint(0.02 * top * rng.random(shp[case.dark])) if case.dark != "none" else None
    fin = oracle_frames = frames
    front = None
    if case.front != "none":
        med = 3 if case.front == "med3bin2" else 0
        raw = np.repeat(np.repeat(frames, 2, axis=1), 2, axis=2).astype(np.int32) + rng.integers(-1, 2, (frames.shape[0], 2 * H, 2 * W))
        raw = np.clip(raw, 0, 255 if case.samples == "u8" else 65535).astype(frames.dtype)
        oracle_frames = np.stack([orc.resize_area(orc.median_blur(f, med) if med else f, 2, 2) for f in raw]).astype(frames.dtype)
        fin, front = raw, (med, 2, 2)
    elif case.samples == "f32":
        fin = frames.astype(np.float32)
    elif case.samples == "f64":
        fin = oracle_frames = np.abs(frames.astype(np.float64) + rng.uniform(-0.5, 0.5, frames.shape))
        assert not np.any(fin == np.rint(fin))
    phase = synth.dispersion_phase(fam.geometry["numfftpoints"]) if case.phase == "on" else None
    window = hamming(W) if case.window == "hamming" else None
    for a in (fin, oracle_frames, yb, yp, yd, phase, window):
        if a is not None:
            a.setflags(write=False)
    return Inputs(config(fam, case), fin, oracle_frames, yb, yp, yd, phase, window, int(case.bandpass == "on"), front)


def _reference_of_doubles(i, truth):
    """helpers.oracle_reference for frames of doubles: the driver of oracle/fdoct_oracle.c (process_u16_impl, orc_finish) over
    orc.frame_to_mag.  (mag (G, H, D) with the epsilon, dB (G, H, D))."""
    import oracle_lib as orc
    cfg = i.cfg
    W, H, N, D, M, A = cfg.width, cfg.height, cfg.numfftpoints, cfg.numdisplaypoints, cfg.increasefftpointsmultiplier, cfg.averages
    sim = cfg.variant == VARIANT_SIM
    p = orc.make_params(W, H, N, D, M, rowwisenormalize=cfg.rowwisenormalize, donotnormalize=0 if sim else cfg.donotnormalize,
                        movavgn=cfg.movavgn, bandpass=i.bandpass, truth=truth)
    win = orc.barthann(W) if i.window is None else i.window
    idx, frac = orc.tables(W, M, N, cfg.lambdamin, cfg.lambdamax)
    eps = 1e-6 if sim else 1e-5
    G = i.oracle_frames.shape[0] // A
    mag = np.empty((G, H, D))
    for g in range(G):
        group = [np.asarray(orc.frame_to_mag(p, i.oracle_frames[g * A + a], i.yb, i.yp, win, idx, frac, yd=i.yd, phase=i.phase), np.float64)[:, :D]
                 for a in (range(A - 1, A) if sim else range(A))]
        mag[g] = sum(group) / len(group) + eps
    db = 20.0 * np.log(mag) / 2.303
    if D > 4:
        db[..., 0] = db[..., 1] = db[..., 4]
    return mag, db


@functools.lru_cache(maxsize=64)
def reference(fam_name, case):
    """(mag_o, db_o, mag_t, db_t): the f32 restatement and the chain in double of a case, (G, H, D) each, computed once and shared."""
    import helpers
    i = inputs(fam_name, case)
    if i.oracle_frames.dtype == np.float64:
        out = _reference_of_doubles(i, 0) + _reference_of_doubles(i, 1)
    else:
        kw = dict(yp=i.yp, yd=i.yd, window=i.window, phase=i.phase, bandpass=i.bandpass)
        mag_o, _, db_o = helpers.oracle_reference(i.cfg, i.oracle_frames, i.yb, _register=False, **kw)
        mag_t, _, db_t = helpers.oracle_truth(i.cfg, i.oracle_frames, i.yb, _register=False, **kw)
        out = (mag_o, np.ascontiguousarray(np.transpose(db_o, (0, 2, 1))), mag_t, np.ascontiguousarray(np.transpose(db_t, (0, 2, 1))))
    for a in out:
        a.setflags(write=False)
    return out


def oracle_distance(fam_name, case):
    """|f32 restatement - chain in double| / tolerance, the worst bin."""
    import helpers
    mag_o, _, mag_t, _ = reference(fam_name, case)
    return float(helpers.mag_ratio(mag_o, mag_t).max())


# ---- the call as make_route sees it (tests/native/option_pairs_route.cpp) ----------------------------------------------------------------
OFFGRID_BYTES = 4        # the base of each output, and of the frames, off the 16-byte grid


def frames_offset(case):
    """Bytes between the 16-byte grid and the first sample of an offgrid call: 4, and 8 for doubles (their own alignment)."""
    if case.entry != "offgrid":
        return 0
    return 8 if case.samples == "f64" else OFFGRID_BYTES


def device_pitch(fam, case):
    """Row pitch in bytes of the frames of a device-pointer call: packed rows, or (offgrid) the next multiple of 4 bytes that is no
    multiple of 16."""
    es = {"u8": 1, "u16": 2, "f32": 4, "f64": 8}[case.samples]
    row = es * shape(fam)[0] * (1 if case.front == "none" else 2)
    if case.entry != "offgrid":
        return row
    pitch = (row + 3) // 4 * 4 + 4
    if es == 8:
        pitch = (row + 8)            # (f64 rows: a multiple of 8, fdoct_route_value.cpp:173)
    return pitch + (4 if es < 8 else 8) if pitch % 16 == 0 else pitch


def route_line(fam, case):
    """The 29 integers of a call for tests/native/option_pairs_route.cpp."""
    W, M, N = shape(fam)
    A = library_averages(case)
    es = {"u8": 1, "u16": 2, "f32": 4, "f64": 8}[case.samples]
    fe = 1 if case.front == "none" else 2
    host = case.entry == "host"
    row = es * W * fe
    # host arrays are staged packed to 16 bytes at an aligned address; the sim variant's last frames are gathered to an aligned
    # workspace with the caller's pitch
    pitch = (row + 15) // 16 * 16 if host and not (case.norm == "sim" and case.averages > 1) else row if host else device_pitch(fam, case)
    off = 0 if case.norm == "sim" and case.averages > 1 else frames_offset(case)
    out_off = OFFGRID_BYTES if case.entry == "offgrid" else 0
    normalize = case.norm in ("whole", "sim")
    return [W, M, N, display_points(fam, case.display), fam.H, A, GROUPS * A, {"u8": 0, "u16": 1, "f32": 2, "f64": 3}[case.samples],
            fam.H if case.background == "frame" else 1, int(case.pi != "none"), int(case.dark != "none"), int(case.bandpass == "on"),
            int(case.norm == "rowwise"), int(normalize), int(case.phase == "on"), case.movavgn,
            3 if case.front == "med3bin2" else 0, fe, 1, int(fam.setup == "staged"), -3 if fam.setup == "rows-in-hbm" else -1,
            int(fam.setup == "any-option"), int(case.division == "two"), 2 if case.launch == "grid2" else 0, off, pitch,
            out_off if case.outputs != "db" else -1, out_off if case.outputs != "bscan" else -1, int(case.layout == "DxH")]
