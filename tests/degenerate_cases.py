"""The degenerate frames and planes of tests/test_gpu_degenerate_inputs.py, and the kernel families they are put through, as plain
numpy: what a real instrument hands the chain besides well-behaved interferograms -- dark rows, saturated rows, rows without
fringes, single hot pixels, dead detector columns, a background captured with a blocked line.  tests/test_degenerate_cases.py
holds every case to its conditions on the CPU (the rows are what they are called, the oracle stays finite, its empty rows are the
ones named here, the f32 restatement itself lies within helpers.TRUTH_LIMIT of the chain in double); the GPU tests run the same
cases through every kernel family.

A frame has 11 rows -- no multiple of four, so on the 512-point plan (four rows per wave) degenerate and ordinary rows share waves:

  row 0   an ordinary synth row                 row 6   one sample of `top` at column W - 2
  row 1   all zeros                             row 7   one sample of `top` on a column where the background is zero
  row 2   all `top`                                     (column W // 2; on the clean background just a third impulse)
  row 3   a constant mid value                  row 8   alternating 0 / `top`
  row 4   the background row itself: no fringe  row 9   a second, different ordinary row
  row 5   one sample of `top` at column 1       row 10  a copy of row 0

`top` is 65535 (16-bit samples) or 255 (8-bit samples)."""
import collections
import functools

import numpy as np

from fdoct_amd import VARIANT_MAIN, VARIANT_SIM, Config, capi, synth

ROWS = 11
ORDINARY, ZEROS, TOP, MID, NO_FRINGE, IMPULSE_LEFT, IMPULSE_RIGHT, IMPULSE_DEAD, ALTERNATING, ORDINARY_2, COPY = range(ROWS)
DEGENERATE = (ZEROS, TOP, MID, NO_FRINGE, IMPULSE_LEFT, IMPULSE_RIGHT, IMPULSE_DEAD, ALTERNATING)
SYNTH_FRAME = 3          # synth.make_frame's frame number of the ordinary rows
ONE_COLUMN = 7           # the background column of value 1: a quotient of full scale next to ordinary ones
BLOCKED_ROW = ORDINARY_2  # the all-zero row of the full-frame background: under an ordinary frame row


def dead_columns(W):
    return [0, W // 2, W - 1]


def mid_value(top):
    return (top + 1) // 4 + 3


def _dtype(top):
    assert top in (255, 65535)
    return np.uint8 if top == 255 else np.uint16


def ordinary_rows(W, H, top):
    return synth.make_frame(SYNTH_FRAME, W, H, dtype=_dtype(top))


def frame_rows(W, yb_row, top, H=ROWS):
    """One frame of the 11 rows above (H > 11: followed by H - 11 ordinary ones).  yb_row: the background row, in sample counts,
    that row 4 repeats and whose zero column row 7 hits."""
    yb_row = np.asarray(yb_row, np.float64)
    assert yb_row.shape == (W,) and H >= ROWS
    f = ordinary_rows(W, H, top)
    f[ZEROS] = 0
    f[TOP] = top
    f[MID] = mid_value(top)
    f[NO_FRINGE] = np.clip(np.rint(yb_row), 0, top).astype(f.dtype)
    for r, c in ((IMPULSE_LEFT, 1), (IMPULSE_RIGHT, W - 2), (IMPULSE_DEAD, W // 2)):
        f[r] = 0
        f[r, c] = top
    f[ALTERNATING] = 0
    f[ALTERNATING, 1::2] = top
    f[COPY] = f[ORDINARY]
    return f


def background(kind, W, H, top):
    """In sample counts, integer-valued (so that row 4 repeats it exactly).  'clean': the rounded synth background, all positive.
    'dead': zeros at columns 0, W // 2 and W - 1 and the value 1 at column 7.  'full': H x W, the clean row scaled per row as the
    2-D tests of test_gpu_parity.py do, with the same dead columns and one all-zero row."""
    row = synth.make_background(W, dtype=_dtype(top)).astype(np.float64)
    assert row.min() > 0
    if kind == "clean":
        return row
    if kind == "dead":
        row[dead_columns(W)] = 0.0
        row[ONE_COLUMN] = 1.0
        return row
    assert kind == "full"
    rng = np.random.default_rng(17)
    full = np.clip(np.rint(row[None, :] * (0.8 + 0.4 * rng.random((H, 1)))), 1.0, top)
    full[:, dead_columns(W)] = 0.0
    full[:, ONE_COLUMN] = 1.0
    full[BLOCKED_ROW] = 0.0
    return full


def pi_frame(frame):
    """A pi frame equal to the frame: the difference is zero everywhere."""
    return frame.astype(np.float64)


def dark_frame(frame, top):
    """Above the frame on the even rows -- one and a half times the row plus a little noise, so the samples are negative after the
    subtraction -- and a little noise alone on the odd ones.  The copy of row 0 gets row 0's dark row."""
    rng = np.random.default_rng(41)
    H, W = frame.shape
    yd = 0.02 * top * rng.random((H, W))
    yd[0::2] += 1.5 * frame[0::2]
    yd[COPY] = yd[ORDINARY]
    return yd


def constant_frame(W, H, top):
    """Whole-frame normalisation: range 0, scale 0, every output row pure epsilon."""
    return np.full((H, W), mid_value(top), _dtype(top))


def corners_frame(W, H, top):
    """Whole-frame normalisation: the only 0 is the first sample, the only `top` the last one."""
    f = np.clip(synth.make_frame(SYNTH_FRAME + 1, W, H, dtype=_dtype(top)), 1, top - 1)
    f[0, 0] = 0
    f[-1, -1] = top
    return f


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# opt     'plain' | 'rowwise' (rowwisenormalize) | 'whole' (donotnormalize = 0) | 'sim' (the sim variant: whole-frame, eps 1e-6)
# bg      'clean' | 'dead' | 'full'
# frames  'one' | 'pair' (averages = 2, the second frame all zero) | 'constant' | 'corners' (the last two: whole-frame normalisation)
# extra   None | 'pi' | 'dark'
# bits    16 | 8
Case = collections.namedtuple("Case", "opt bg frames extra bits", defaults=("one", None, 16))
C = Case

FAST = [C("plain", "clean"), C("plain", "dead"), C("plain", "full"), C("rowwise", "clean"), C("rowwise", "full"), C("whole", "dead"),
        C("whole", "full"), C("whole", "clean", "constant"), C("whole", "clean", "corners"), C("sim", "clean"),
        C("plain", "dead", "pair"), C("plain", "full", "pair"), C("plain", "dead", bits=8), C("rowwise", "full", bits=8)]
# the chain's own D x H store is compiled for the plain and the averaging kernel, and on the 1024-point plan for a full-frame
# background and the whole-frame normalisation of one frame per B-scan (fdoct_launch.cpp: tro_configured)
FAST_DXH = [C("plain", "clean"), C("plain", "dead"), C("plain", "full"), C("whole", "dead"), C("whole", "full"),
            C("whole", "clean", "corners"), C("plain", "dead", "pair"), C("plain", "full", bits=8)]
FAST_DXH_512 = [C("plain", "clean"), C("plain", "dead"), C("plain", "dead", "pair"), C("plain", "dead", bits=8)]
# the whole-frame frames: 'constant' drives every family's own 0-or-1/(max - min) guard to 0, 'corners' puts the extremes at the
# first and the last sample the pre-pass reads
_FRAME_NORM = [C("whole", "clean", "constant"), C("whole", "clean", "corners")]
ANY_OPTION = [C("plain", "clean"), C("plain", "dead", extra="pi"), C("plain", "dead", extra="dark"), C("rowwise", "full"),
              C("whole", "dead"), C("sim", "clean"), C("plain", "full", "pair"), C("sim", "clean", "constant")] + _FRAME_NORM
# staged mode is built for the plain 16-bit configuration only (fdoct_launch.cpp: no normalisation, no full-frame background)
STAGED = [C("plain", "clean"), C("plain", "dead"), C("plain", "dead", "pair"), C("plain", "clean", "pair")]
WAVE = [C("plain", "clean"), C("plain", "dead"), C("plain", "full"), C("plain", "dead", "pair"), C("rowwise", "dead"), C("whole", "clean"),
        C("plain", "dead", extra="pi"), C("plain", "clean", extra="dark")] + _FRAME_NORM
WAVE_U8 = [C("plain", "clean", bits=8), C("plain", "dead", bits=8), C("plain", "full", bits=8), C("plain", "dead", "pair", bits=8),
           C("rowwise", "full", bits=8), C("whole", "dead", bits=8), C("whole", "clean", "constant", bits=8)]
WAVE_JIT = [C("plain", "clean"), C("plain", "dead"), C("rowwise", "full"), C("whole", "dead"), C("plain", "dead", extra="dark"),
            C("plain", "dead", extra="pi"), C("plain", "full", "pair")] + _FRAME_NORM
GENERIC = [C("plain", "clean"), C("plain", "dead"), C("plain", "full"), C("rowwise", "dead"), C("whole", "full"), C("sim", "clean"),
           C("plain", "dead", "pair"), C("plain", "dead", extra="pi"), C("plain", "clean", extra="dark"), C("plain", "dead", bits=8),
           C("sim", "clean", "constant")] + _FRAME_NORM
BLUESTEIN = [C("plain", "clean"), C("plain", "dead"), C("rowwise", "full"), C("whole", "dead"), C("plain", "dead", "pair")] + _FRAME_NORM
WG1024 = [C("plain", "clean"), C("plain", "dead"), C("rowwise", "full"), C("whole", "dead"), C("plain", "dead", "pair"),
          C("plain", "clean", extra="dark")] + _FRAME_NORM
# (the oracle takes about a second per frame of these rows: five frames)
LONG = [C("plain", "clean", "pair"), C("rowwise", "full")] + _FRAME_NORM

HXD, DXH = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
Family = collections.namedtuple("Family", "name geometry H setup layout kernel cases")
_JIT_RANGE = dict(lambdamin=840.5e-9, lambdamax=859.5e-9)


def _geo(W, N, D, M=1, **kw):
    return dict(width=W, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, **kw)


# setup: None | 'any-option' (set_plan(-1, True)) | 'staged' (set_staged(True)).  kernel: what last_kernel() must report -- for the
# wave-per-row kernel's built-in shapes the run-time compiled one wherever an option is on (they are its compile-time options).
FAMILIES = [
    Family("fused fast path, 512-point plan", _geo(1024, 1024, 512), ROWS, None, HXD, capi.KERNEL_FUSED, FAST),
    Family("fused fast path, 1024-point plan", _geo(2048, 2048, 1024), ROWS, None, HXD, capi.KERNEL_FUSED, FAST),
    Family("fused fast path, 2048-point plan", _geo(4096, 4096, 2048), ROWS, None, HXD, capi.KERNEL_FUSED, FAST),
    Family("fused fast path, D x H, 1024-point plan", _geo(2048, 2048, 1024), 20, None, DXH, capi.KERNEL_FUSED_TRANSPOSED, FAST_DXH),
    Family("fused fast path, D x H, 512-point plan", _geo(1024, 1024, 512), 20, None, DXH, capi.KERNEL_FUSED_TRANSPOSED, FAST_DXH_512),
    Family("fused any-option kernel", _geo(2048, 2048, 1024), ROWS, "any-option", HXD, capi.KERNEL_FUSED, ANY_OPTION),
    Family("fused, staged", _geo(2048, 2048, 1024), ROWS, "staged", HXD, capi.KERNEL_FUSED_STAGED, STAGED),
    Family("wave-per-row, 160 x 4", _geo(160, 2560, 320, 4), ROWS, None, HXD, capi.KERNEL_WAVE, WAVE),
    Family("wave-per-row, 640 x 1, 8-bit", _geo(640, 640, 320), ROWS, None, HXD, capi.KERNEL_WAVE, WAVE_U8),
    Family("wave-per-row, run-time compiled, 200 x 4", _geo(200, 2560, 320, 4, **_JIT_RANGE), ROWS, None, HXD, capi.KERNEL_WAVE_JIT, WAVE_JIT),
    Family("workgroup-per-row, 2048 -> 2002", _geo(2048, 2002, 1001), ROWS, None, HXD, capi.KERNEL_GENERIC, GENERIC),
    Family("workgroup-per-row, Bluestein, 322 x 4", _geo(322, 1288, 320, 4), ROWS, None, HXD, capi.KERNEL_GENERIC, BLUESTEIN),
    Family("workgroup-per-row, 1024 threads, 2400 x 4", _geo(2400, 9600, 1000, 4), ROWS, None, HXD, capi.KERNEL_GENERIC, WG1024),
    Family("long rows, 2048 x 8", _geo(2048, 65536, 2048, 8), ROWS, None, HXD, capi.KERNEL_LONG_ROWS, LONG),
]
FAMILY_IDS = [f.name for f in FAMILIES]


def family(name):
    return FAMILIES[FAMILY_IDS.index(name)]


def wave_option(case):
    """Whether the case turns on one of the wave-per-row kernel's compile-time options (fdoct_route_value.cpp: wave_opt)."""
    return case.opt != "plain" or case.extra is not None


def expected_kernel(fam, case):
    if fam.kernel == capi.KERNEL_WAVE and wave_option(case):
        return capi.KERNEL_WAVE_JIT
    return fam.kernel


def config(fam, case):
    return Config(height=fam.H, averages=2 if case.frames == "pair" else 1, rowwisenormalize=int(case.opt == "rowwise"),
                  donotnormalize=0 if case.opt == "whole" else 1, variant=VARIANT_SIM if case.opt == "sim" else VARIANT_MAIN,
                  **fam.geometry)


def eps_of(case):
    return 1e-6 if case.opt == "sim" else 1e-5


Inputs = collections.namedtuple("Inputs", "cfg frames yb yp yd")


@functools.lru_cache(maxsize=None)
def inputs(fam_name, case):
    """The frames (u16 / u8, (1 or 2, H, W)), the background as the handle takes it and the pi / dark frames of a case."""
    fam = family(fam_name)
    W, H = fam.geometry["width"], fam.H
    top = 255 if case.bits == 8 else 65535
    yb = background(case.bg, W, H, top)
    frame = frame_rows(W, yb[NO_FRINGE] if yb.ndim == 2 else yb, top, H)
    if case.frames == "constant":
        frame = constant_frame(W, H, top)
    elif case.frames == "corners":
        frame = corners_frame(W, H, top)
    assert case.frames in ("one", "pair") or case.opt in ("whole", "sim")
    assert case.extra is None or (case.opt == "plain" and case.frames == "one" and case.bg != "full")
    frames = np.stack([frame, np.zeros_like(frame)]) if case.frames == "pair" else frame[None]
    if case.opt != "plain":
        yb = yb / top                       # the normalisations leave samples in [0, 1]
    yp = pi_frame(frame) if case.extra == "pi" else None
    yd = dark_frame(frame, top) if case.extra == "dark" else None
    for a in (frames, yb, yp, yd):
        if a is not None:
            a.setflags(write=False)
    return Inputs(config(fam, case), frames, yb, yp, yd)


def empty_rows(case, H=ROWS):
    """The output rows the chain leaves empty -- nothing but its epsilon in every bin."""
    if case.extra == "pi" or case.frames == "constant":
        return list(range(H))
    rows = set()
    if case.bg == "full":
        rows.add(BLOCKED_ROW)                       # x / 0 = 0 along the whole row
    if case.frames in ("one", "pair") and case.extra is None:
        rows.add(ZEROS)
        if case.opt == "rowwise":
            rows.update((TOP, MID))                 # range 0: scale 0
        elif case.bg == "clean":
            rows.add(NO_FRINGE)                     # the quotient is 1 in every column; its mean removed, nothing is left
        if case.bg != "clean":
            rows.add(IMPULSE_DEAD)                  # the row's only sample falls on x / 0 = 0
    return sorted(rows)


def dc_level_rows(case):
    """Among the empty rows, those that are empty only because a DC level cancels: the no-fringe row, and the constant rows under
    row-wise normalisation (over a background that is not flat).  Every other empty row holds zeros before any rounding."""
    if case.extra is not None or case.frames not in ("one", "pair"):
        return []
    if case.opt == "rowwise":
        return [TOP, MID]
    return [NO_FRINGE] if case.bg == "clean" else []


# Where the second word of 1/background reaches the kernel as the half-float pattern c0 * rho (fdoct_fused_rules.h: IL16, IL16R;
# fdoct_state.cpp: half_pattern_row): the fast-path kernels with at most 32 samples per lane, and the 512-point plan's without a
# normalisation.  The pattern keeps 11 bits of rho = (1/yb - ib) / ib, |rho| <= 2^-24, so up to 2^-35 of the DC level stays in every
# sample: these kernels cannot leave the no-fringe row within the 1e-9 of pure epsilon, by design.
HALF_PATTERN = {
    "fused fast path, 512-point plan": ("plain",),
    "fused fast path, 1024-point plan": ("plain", "whole", "sim"),
    "fused fast path, D x H, 1024-point plan": ("plain", "whole"),
    "fused fast path, D x H, 512-point plan": ("plain",),
    "fused, staged": ("plain",),
}


def half_pattern(fam_name, case):
    return case.opt in HALF_PATTERN.get(fam_name, ())


@functools.lru_cache(maxsize=None)
def half_pattern_no_fringe_row(fam_name, case):
    """What the half-float form of the second word leaves of the no-fringe row, in double: the quotient is v (ib + c0 rho~) with
    v = yb, ib = fl32(1 / yb), rho~ = rho rounded to a half float at 2^-38 and c0 = 1 up to 2^-24 -- that is 1 + (rho~ - rho) up to
    terms of 2^-48 -- put through the rest of the chain in double.  (D,) linear magnitudes with the chain's epsilon."""
    import oracle_lib as orc
    i = inputs(fam_name, case)
    assert case.bg == "clean" and i.yb.ndim == 1 and NO_FRINGE in dc_level_rows(case)
    cfg = i.cfg
    W, N, D, M = cfg.width, cfg.numfftpoints, cfg.numdisplaypoints, cfg.increasefftpointsmultiplier
    q = 1.0 / i.yb
    ib = q.astype(np.float32).astype(np.float64)
    rho = (q - ib) / ib
    rho_h = np.ldexp(np.ldexp(rho, 38).astype(np.float32).astype(np.float16).astype(np.float64), -38)
    x = 1.0 + (rho_h - rho)
    idx, frac = orc.tables(W, M, N, cfg.lambdamin, cfg.lambdamax)
    mag = orc.frame_to_mag(orc.make_params(W, 1, N, D, M, truth=1), x[None, :], np.ones(W), None, orc.barthann(W), idx, frac)
    return mag[0, :D] / cfg.averages + eps_of(case)


def exact_empty_rows(case, H=ROWS):
    """The empty rows that hold zeros before any rounding in every kernel, and so must equal float32(eps) bit for bit: all of them
    but the no-fringe row (a constant row under row-wise normalisation is multiplied by a scale of exactly 0)."""
    return [r for r in empty_rows(case, H) if not (r == NO_FRINGE and r in dc_level_rows(case))]


def distinct_rows(case):
    """Rows whose results must differ pairwise by more than their tolerance: the two ordinary rows and every degenerate row that
    is not empty."""
    if case.frames not in ("one", "pair"):
        return []
    empty = set(empty_rows(case))
    return [r for r in (ORDINARY, ORDINARY_2) + DEGENERATE if r not in empty]


@functools.lru_cache(maxsize=None)
def reference(fam_name, case):
    """(mag_o, db_o, mag_t, db_t): the f32 restatement and the chain in double of a case, (1, H, D) each, computed once and shared."""
    import helpers
    i = inputs(fam_name, case)
    kw = dict(yp=i.yp, yd=i.yd)
    mag_o, _, db_o = helpers.oracle_reference(i.cfg, i.frames, i.yb, _register=False, **kw)
    mag_t, _, db_t = helpers.oracle_truth(i.cfg, i.frames, i.yb, _register=False, **kw)
    out = (mag_o, np.ascontiguousarray(np.transpose(db_o, (0, 2, 1))), mag_t, np.ascontiguousarray(np.transpose(db_t, (0, 2, 1))))
    for a in out:
        a.setflags(write=False)
    return out


def is_empty(mag_rows, eps):
    """Per row: every bin equals float32(eps) once rounded to the output type."""
    return (np.asarray(mag_rows).astype(np.float32) == np.float32(eps)).all(axis=-1)
