"""The cases of tests/test_gpu_doppler_edges.py, the second pass over the Doppler stage (fdoct_doppler.hip), as data and pure
functions; tests/test_doppler_edge_cases.py holds each to its conditions on the CPU from tests/doppler_model.py alone, as
tests/test_doppler_cases.py does for the first 17 cases.  Fields are doppler_cases.field's.

  seams     pair rows 15 .. 33 x depths 63 .. 129 around the 16 x 64 tile: the last tile's halo is cut at the image;
  windows   every size 1 .. 32 each way as a thin window, the anti-diagonal, 2 x 2 and 31 x 31, and the two sizes on either side
            of 64 KiB of dynamic LDS;
  reach     which outputs a sample can influence: the halo, the lag partner, the image's edge, as one pure function;
  tall      a batch beyond one pass of the capped grid whose pair images have two tiles each way;
  exact     a field on which every product and sum is exact in float, for the mask's strict comparison."""
import numpy as np

import doppler_cases as dc
from doppler_model import ASCANS, FRAMES

TILE_ROWS, TILE_DEPTHS = dc.TILE_ROWS, dc.TILE_DEPTHS


# ---- the launch arithmetic restated (fdoct_boxtile.h: box_lds_bytes, three planes) --------------------------------------------------
def lds_bytes(wa, wd):
    """Three planes of floats of the staged halo tile, (TILE_ROWS + wa - 1) x (TILE_DEPTHS + wd - 1), and three of its depth sums,
    (TILE_ROWS + wa - 1) x TILE_DEPTHS: 12 (15 + wa)(127 + wd)."""
    sr, sw = TILE_ROWS + wa - 1, TILE_DEPTHS + wd - 1
    return 3 * 4 * (sr * sw + sr * TILE_DEPTHS)


LDS_DEFAULT_LIMIT = 64 << 10          # beyond it the launcher raises the kernel's dynamic-LDS limit (LdsGrant)


# ---- a. seams ------------------------------------------------------------------------------------------------------------------------
SEAM_ROWS = (15, 16, 17, 31, 32, 33)            # pair rows: one below, on and one above one and two tiles
SEAM_DEPTHS = (63, 64, 65, 127, 128, 129)


def _seam(pair_rows, D, axis, win, seed, bulk=None):
    H = pair_rows + 1 if axis == ASCANS else pair_rows
    what = "%d x %d, %d pair rows x %d depths, %s lag 1%s" % (win[0], win[1], pair_rows, D, "A-scans" if axis == ASCANS else "frames",
                                                               ", bulk" if bulk else "")
    return dc._case(what, 2, H, D, axis, 1, win, seed, bulk=bulk, speckle=True)


# all 36 shapes on the A-scans axis with the even window 4 x 8 ...
SEAM_CASES = [_seam(pr, D, ASCANS, (4, 8), 100 + 6 * i + j) for i, pr in enumerate(SEAM_ROWS) for j, D in enumerate(SEAM_DEPTHS)]
# ... and twelve on the frames axis with 3 x 5 and the bulk correction: row count i with depths i and i + 3, so that every row
# count meets a depth of the first and of the second tile seam
SEAM_BULK_CASES = [_seam(SEAM_ROWS[i], SEAM_DEPTHS[(i + k) % 6], FRAMES, (3, 5), 200 + 2 * i + k // 3, bulk=True) for i in range(6) for k in (0, 3)]


# ---- b. every window size ------------------------------------------------------------------------------------------------------------
SWEEP_SHAPE, SWEEP_SEED = (2, 21, 70), 300       # 20 pair rows x 70 depths: two tiles each way
WINDOW_GROUPS = {
    "across A-scans": [(w, 1) for w in range(2, 33)],
    "along depth": [(1, w) for w in range(2, 33)],
    "anti-diagonal": [(w, 33 - w) for w in range(1, 33)],
    "squares": [(2, 2), (31, 31)],
    "either side of 64 KiB of LDS": [(20, 29), (20, 30)],    # run in this order, then 1 x 1 again
}
LDS_STRADDLE = ((20, 29), (20, 30))


def sweep_field():
    return dc.field(*SWEEP_SHAPE, SWEEP_SEED, speckle=True)


def sweep_args(win):
    return dict(axis=ASCANS, lag=1, win=win, bulk=None, scale=1.0, min_power=0.0)


# ---- c. reach ------------------------------------------------------------------------------------------------------------------------
REACH_H, REACH_D, REACH_SEED = 34, 130, 400
REACH_WINDOWS = ((4, 8), (1, 1))
REACH_LAGS = (1, 2)


def reach_frames(axis, lag):
    """Two frames on the A-scans axis; on the frames axis 2 lag + 1, the fewest with a frame that is X1 of one pair image and
    X2 of another."""
    return 2 if axis == ASCANS else 2 * lag + 1


def reach_positions(axis, lag):
    """(frame, row, depth) of the poisoned sample: the four corners of the interior tile seam, in the frame that has both
    partners, and the image's first and last sample."""
    n = reach_frames(axis, lag)
    f = 1 if axis == ASCANS else lag
    seam = [(f, r, b) for r in (TILE_ROWS - 1, TILE_ROWS) for b in (TILE_DEPTHS - 1, TILE_DEPTHS)]
    return seam + [(0, 0, 0), (n - 1, REACH_H - 1, REACH_D - 1)]


def reach_configs():
    return [(axis, lag, win) for axis in (ASCANS, FRAMES) for lag in REACH_LAGS for win in REACH_WINDOWS]


def partners(axis, lag, pos, pair_images, pair_rows):
    """(pair image, pair row) of the pairs formed from sample pos = (f, r, b): as X1 at its own index, as X2 `lag` before it."""
    f, r, _ = pos
    both = [(f, r), (f, r - lag)] if axis == ASCANS else [(f, r), (f - lag, r)]
    return [(p, q) for p, q in both if 0 <= p < pair_images and 0 <= q < pair_rows]


def _span(at, w, n):
    """Outputs i whose window [i - (w - 1) // 2, i + w // 2] holds `at`: i in [at - w // 2, at + (w - 1) // 2], cut to [0, n)."""
    return slice(max(at - w // 2, 0), min(at + (w - 1) // 2, n - 1) + 1)


def reach(axis, lag, win, pos, shape, all_depths=False):
    """Boolean (pair_images, pair_rows, depths): the outputs whose window holds a pair formed from sample pos of X of `shape`.
    all_depths: every depth of those rows -- what the bulk correction can move, since the row's phasor is a sum over depth."""
    n, H, D = shape
    pi, pr = (n - lag, H) if axis == FRAMES else (n, H - lag)
    out = np.zeros((pi, pr, D), bool)
    for p, q in partners(axis, lag, pos, pi, pr):
        out[p, _span(q, win[0], pr), slice(None) if all_depths else _span(pos[2], win[1], D)] = True
    return out


def reach_field(axis, lag):
    return dc.field(reach_frames(axis, lag), REACH_H, REACH_D, REACH_SEED + 2 * lag + axis)


def poisoned(X, pos):
    Y = X.copy()
    Y[pos] = np.complex64(complex(np.nan, np.nan))
    return Y


# ---- d. a tall batch with tiles both ways -------------------------------------------------------------------------------------------
# Frames of 18 A-scans x 65 depths.  A-scans, lag 1: 17 pair rows; frames, lag 3: 18 -- two row tiles x two depth tiles a pair
# image on both.  The construction is doppler_cases' tall batch's: period-3 frames, pair image p of the tall result is the base's
# p mod 3.
TALL2_H, TALL2_D, TALL2_WIN = 18, 65, (4, 8)
TALL2_BASE = dc.TALL_BASE                        # axis: (base frames, lag)
TALL2_BULK = {ASCANS: True, FRAMES: None}        # the bulk kernel loops on one axis; the other runs the stage alone


def tall2_shape(axis, n):
    _, lag = TALL2_BASE[axis]
    return (n - lag, TALL2_H) if axis == FRAMES else (n, TALL2_H - lag)


def tall2_ok(axis, n, cus):
    pi, pr = tall2_shape(axis, n)
    rows_ok = dc.beyond(pi * pr, dc.grid_cap(cus)) if TALL2_BULK[axis] else True
    return n % 3 == 0 and dc.beyond(dc.tiles(pi, pr, TALL2_D), dc.grid_cap(cus)) and rows_ok


def tall2_frames(axis, cus):
    """The fewest frames, a multiple of 3, whose tiles -- and pair rows, where the bulk kernel runs -- go beyond one pass."""
    base_n, _ = TALL2_BASE[axis]
    for n in range(base_n + 3, base_n + 3 + 3 * 100000, 3):
        if tall2_ok(axis, n, cus):
            return n
    raise ValueError("no tall batch for %d CUs" % cus)


def tall2_base_ok(axis, cus):
    pi, pr = tall2_shape(axis, TALL2_BASE[axis][0])
    return dc.tiles(pi, pr, TALL2_D) <= dc.grid_cap(cus) and pi * pr <= dc.grid_cap(cus)


# ---- e. an exact field ---------------------------------------------------------------------------------------------------------------
EXACT_WINDOWS = ((1, 1), (2, 2), (3, 5), (4, 8))
EXACT_POWER = 25.0                               # |3 + 4j|^2


def exact_field(n=SWEEP_SHAPE[0], H=SWEEP_SHAPE[1], D=SWEEP_SHAPE[2]):
    """X[f, r, b] = (3 + 4j) i^r: every lag-1 product along A-scans is 25 i, every |X|^2 is 25, and every sum of at most 1024
    of them is an integer below 2^24 -- exact in float."""
    turn = np.array([1, 1j, -1, -1j], np.complex64)[np.arange(H) % 4]
    return np.ascontiguousarray(np.broadcast_to((np.complex64(3 + 4j) * turn)[None, :, None], (n, H, D))).astype(np.complex64)


# ---- behind the chain (tests/test_gpu_doppler_chain.py) ----------------------------------------------------------------------------
CHAIN_DEPTHS = (1, 63, 64, 65)


def option_axes(case):
    """[(axis, bulk)] an option case of tests/complex_cases.py is run with: kind k takes axis k mod 2 with the bulk correction on its
    wave form and the other axis without it on its generic form, so that every kind meets both axes and both settings; the
    four-bit case, which has a wave form only, takes both."""
    import complex_cases as cc
    if case.kind == cc.FOUR_BITS:
        return [(ASCANS, True), (FRAMES, None)]
    k = cc.KINDS.index(case.kind)
    return [((k + (case.route == "generic")) % 2, True if case.route == "wave" else None)]


def chain_depth_cases():
    import complex_cases as cc
    return [c for c in cc.DEPTH_CASES if c.D in CHAIN_DEPTHS]
