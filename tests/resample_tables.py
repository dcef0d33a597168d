"""Caller-supplied lambda -> k resample tables (fdoct_set_resample_table, fdoct_set_lambda_range) and the kernel families they are
put through by tests/test_gpu_resample_tables.py, as plain numpy.  tests/test_resample_tables.py holds every table and every
(family, table) pair to its conditions on the CPU.

What the tables are for: every table the library builds itself (BscanFFT.cpp:615-698) for the ranges the suite uses looks the same
to a kernel.  Over the gathered entries q = 1 .. N-2 nearestkindex walks slowly down the row (steps of 0 .. -5), never reaches
sample 0, stays a few samples below M W - 1, and fractionalk lies in (0, 1].  So the slopes[0] = slopes[1] rule (main:1161), the
column M W - 1 that an odd width under an even multiplier does not have, any gather that is not a slow monotone walk, and the
folded window planes for fractionalk outside [0, 1] are never observed with the built tables.  The tables here reach them:

  wide           the built table for 400 - 1000 nm, given through fdoct_set_lambda_range: the other setter; curvature
  ends           an ascending gather from sample 0 to sample M W - 1, fractionalk[0] = 0.37 and fractionalk[M W - 1] = 0.61
  reversed       the built table read back to front
  evenodd        its even entries, then its odd ones: one jump back across the row, the halves of every packed pair far apart
  sawtooth       four ascending ramps over the whole row
  held           every source repeated for eight outputs
  extrapolating  the built nearestkindex with fractionalk uniform in [-0.5, 1.5]
  ends+hamming   `ends` under a Hamming window (fdoct_set_window).  The Bartlett-Hann window is 0 at sample 0 and 2e-4 at sample
                 1: under it the slopes[0] = slopes[1] rule moves data_ylin[1] of an ORDINARY row by 0.01 - 0.9 x the tolerance
                 of a bin on most geometries, which no parity check can tell from rounding (there the frame's degenerate rows --
                 the saturated row, the impulse at column 1 -- carry it).  The Hamming window is 0.08 at both ends: there the
                 rule is worth 10 - 200 x the tolerance on an ordinary row of every family but the 65536-point long rows
                 (slope_rule_weight; asserted in tests/test_resample_tables.py)

Entries 0 and N - 1 of a table are never read by the chain (main:1164); they hold a legal value.  fractionalk is indexed by
SAMPLE (fractionalk[nearestkindex[q]], main:1167-1173), 0 past its end.

The families: every entry of degenerate_cases.FAMILIES with its plain 16-bit case on the clean background (8-bit where the family
is an 8-bit one) -- rows 0 and 9 of its 11-row frame are ordinary, the degenerate rows ride along -- and seven more: an odd width
under the full-length zero-pad, in LDS and with the rows in HBM (161 x 4: `ends` reads the column that does not exist, defined
0), M W > N (1280 x 4 -> 2560: fractionalk indexed past its end), the wave-per-row kernel with its tables resident in registers
(640 x 4), and the complex path (dispersion phase) of the fused, the wave-per-row and the workgroup-per-row kernel.  The 65536-point
long-row family takes `ends`, `reversed`, `sawtooth` and `ends+hamming`, every other family all eight.

No (family, table) pair had to be dropped: each holds the f32 restatement within ORACLE_LIMIT of the chain in double."""
import collections
import functools

import numpy as np

import degenerate_cases as dg
from fdoct_amd import Config, capi, synth

WIDE_RANGE = (400e-9, 1000e-9)
TABLES = ("wide", "ends", "reversed", "evenodd", "sawtooth", "held", "extrapolating", "ends+hamming")
LONG_TABLES = ("ends", "reversed", "sawtooth", "ends+hamming")
ORACLE_LIMIT = 0.25      # of the tolerance: half of helpers.TRUTH_LIMIT, so that on the GPU the 0.5 governs
FRAC_AT_0, FRAC_AT_LAST = 0.37, 0.61
HELD = 8
CASE = dg.C("plain", "clean")


def default_table(W, M, N, lambdamin, lambdamax):
    import oracle_lib as orc
    return orc.tables(W, M, N, lambdamin, lambdamax)


def window(name, W):
    """The window a table is run under: None (the built Bartlett-Hann window) or, for 'NAME+hamming', a Hamming window."""
    if not name.endswith("+hamming"):
        return None
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1))


def table(name, W, M, N, lambdamin=Config.lambdamin, lambdamax=Config.lambdamax):
    """(nearestkindex int32[N], fractionalk float64[N]) of the table `name` for W x M samples and N points; lambdamin / lambdamax:
    the range of the built table the others start from."""
    name = name.split("+")[0]
    MW = M * W
    idx0, frac0 = default_table(W, M, N, lambdamin, lambdamax)
    q = np.arange(N, dtype=np.int64)
    idx, frac = idx0.copy(), frac0.copy()
    if name == "wide":
        idx, frac = default_table(W, M, N, *WIDE_RANGE)
    elif name == "ends":
        idx[1:N - 1] = np.rint((q[1:N - 1] - 1) * (MW - 1) / (N - 3)).astype(np.int32)
        frac[0] = FRAC_AT_0
        if MW - 1 < N:
            frac[MW - 1] = FRAC_AT_LAST
    elif name == "reversed":
        idx = idx0[::-1].copy()
    elif name == "evenodd":
        idx = np.concatenate([idx0[0::2], idx0[1::2]])
    elif name == "sawtooth":
        idx = ((4 * q * MW // N) % MW).astype(np.int32)
    elif name == "held":
        idx = idx0[q - q % HELD].copy()
    elif name == "extrapolating":
        frac = np.random.default_rng(1161).uniform(-0.5, 1.5, N)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(frac, np.float64)


# ---- the families ------------------------------------------------------------------------------------------------------------------
# as degenerate_cases.Family, with: phase (the complex path), bits (of the samples), tables; one more setup, 'rows-in-hbm'
# (set_plan(-3): the long-row path for a row that would fit the LDS)
Family = collections.namedtuple("Family", "name geometry H setup layout kernel phase bits tables")


def _from_degenerate(f):
    bits = 8 if all(c.bits == 8 for c in f.cases) else 16
    return Family(f.name, f.geometry, f.H, f.setup, f.layout, f.kernel, False, bits, LONG_TABLES if f.kernel == capi.KERNEL_LONG_ROWS else TABLES)


FAMILIES = [_from_degenerate(f) for f in dg.FAMILIES] + [
    Family("workgroup-per-row, full-length zero-pad, 161 x 4", dg._geo(161, 644, 160, 4), dg.ROWS, None, dg.HXD, capi.KERNEL_GENERIC, False, 16, TABLES),
    Family("rows in HBM, 161 x 4", dg._geo(161, 644, 160, 4), dg.ROWS, "rows-in-hbm", dg.HXD, capi.KERNEL_LONG_ROWS, False, 16, TABLES),
    Family("wave-per-row, 1280 x 4 -> 2560", dg._geo(1280, 2560, 320, 4), dg.ROWS, None, dg.HXD, capi.KERNEL_WAVE, False, 16, TABLES),
    Family("wave-per-row, 640 x 4, tables in registers", dg._geo(640, 2560, 320, 4), dg.ROWS, None, dg.HXD, capi.KERNEL_WAVE, False, 16, TABLES),
    Family("fused, complex rows, 2048 -> 2048, D 700", dg._geo(2048, 2048, 700), dg.ROWS, None, dg.HXD, capi.KERNEL_FUSED, True, 16, TABLES),
    Family("wave-per-row, complex rows, 160 x 4", dg._geo(160, 2560, 320, 4), dg.ROWS, None, dg.HXD, capi.KERNEL_WAVE_JIT, True, 16, TABLES),
    Family("workgroup-per-row, complex rows, 2048 -> 2002", dg._geo(2048, 2002, 1001), dg.ROWS, None, dg.HXD, capi.KERNEL_GENERIC, True, 16, TABLES),
]
FAMILY_IDS = [f.name for f in FAMILIES]
# one family of each table set, for the setter's own contract
SETTER_FAMILIES = ["fused fast path, 1024-point plan", "wave-per-row, 160 x 4", "wave-per-row, run-time compiled, 200 x 4",
                   "workgroup-per-row, 2048 -> 2002", "long rows, 2048 x 8"]


def family(name):
    return FAMILIES[FAMILY_IDS.index(name)]


def shape(fam):
    g = fam.geometry
    return g["width"], g["increasefftpointsmultiplier"], g["numfftpoints"], g["numdisplaypoints"]


Inputs = collections.namedtuple("Inputs", "cfg frames yb phase")


@functools.lru_cache(maxsize=None)
def inputs(fam_name):
    """The configuration, the one frame ((1, H, W), 16- or 8-bit), the one-row background and the dispersion phasors (or None)."""
    fam = family(fam_name)
    W, M, N, D = shape(fam)
    case = CASE._replace(bits=fam.bits)
    if fam_name in dg.FAMILY_IDS:
        i = dg.inputs(fam_name, case)
        cfg, frames, yb = i.cfg, i.frames, i.yb
    else:       # the same rows, as degenerate_cases.inputs makes them
        top = 255 if fam.bits == 8 else 65535
        yb = dg.background(case.bg, W, fam.H, top)
        frames = dg.frame_rows(W, yb, top, fam.H)[None]
        cfg = Config(height=fam.H, **fam.geometry)
        for a in (frames, yb):
            a.setflags(write=False)
    phase = synth.dispersion_phase(N) if fam.phase else None
    return Inputs(cfg, frames, yb, phase)


@functools.lru_cache(maxsize=None)
def family_table(fam_name, name):
    """The table `name` for a family's geometry, started from the table built for the family's own range."""
    cfg = inputs(fam_name).cfg
    W, M, N, _ = shape(family(fam_name))
    idx, frac = table(name, W, M, N, cfg.lambdamin, cfg.lambdamax)
    idx.setflags(write=False)
    frac.setflags(write=False)
    return idx, frac


def gathered(idx):
    """The entries the chain reads: q = 1 .. N - 2 (main:1164)."""
    return np.asarray(idx)[1:-1]


@functools.lru_cache(maxsize=None)
def reference(fam_name, name):
    """(mag_o, db_o, mag_t, db_t): the f32 restatement and the chain in double of a family under a table, (1, H, D) each, computed
    once and shared."""
    import helpers
    i = inputs(fam_name)
    kw = dict(table=family_table(fam_name, name), phase=i.phase, window=window(name, i.cfg.width))
    mag_o, _, db_o = helpers.oracle_reference(i.cfg, i.frames, i.yb, _register=False, **kw)
    mag_t, _, db_t = helpers.oracle_truth(i.cfg, i.frames, i.yb, _register=False, **kw)
    out = (mag_o, np.ascontiguousarray(np.transpose(db_o, (0, 2, 1))), mag_t, np.ascontiguousarray(np.transpose(db_t, (0, 2, 1))))
    for a in out:
        a.setflags(write=False)
    return out


def slope_rule_weight(fam_name, name):
    """What the slopes[0] = slopes[1] rule is worth under a table that gathers sample 0 at q = 1: |data_ylin[1] - what the general
    formula y[0] + g (y[0] - y[-1]) with y[-1] = 0 gives|, which reaches every bin of the transform undiminished, over the smallest
    tolerance of a displayed bin; for the two ordinary rows."""
    import oracle_lib as orc
    fam = family(fam_name)
    W, M, N, D = shape(fam)
    i = inputs(fam_name)
    idx, frac = family_table(fam_name, name)
    assert idx[1] == 0
    win = window(name, W)
    y = i.frames[0].astype(np.float64) / i.yb[None, :]
    y = (y - y.mean(axis=1, keepdims=True)) * (orc.barthann(W) if win is None else win)
    if M > 1:
        y = orc.zeropadrowwise(y, M)
    rows = [dg.ORDINARY, dg.ORDINARY_2]
    delta = np.abs(frac[0] * (y[rows, 1] - y[rows, 0]) - frac[0] * y[rows, 0])
    mag_t = np.abs(reference(fam_name, name)[2][0, rows])
    tol = 1e-4 * mag_t + 1e-6 * mag_t.max(axis=-1, keepdims=True)
    return delta / tol.min(axis=-1)
