"""The 1024-point fast path (W = N = 2048, D = 1024, u16: the benchmark's plan) on rows and batches where its two wave-wide
sums and its row ticket can go wrong.

A wave sums over its 64 lanes twice per row -- the reference sample's mean c0 and the mean of the row -- as a DPP chain: four
row shifts inside each 16-lane group, then row_bcast:15 into groups 1 and 3 and row_bcast:31 into groups 2 and 3; lane 63
holds the total.  Lane l owns samples 8 l .. 8 l + 7 of each 512-sample quarter of the row.  A wrong row mask or broadcast
drops or doubles a group's share of a sum, so the rows here put everything that distinguishes a row from a flat one into one
16-lane group (one row for each of the four), or into the lanes on either side of a group boundary (15 / 16, 31 / 32, 47 / 48)
and lane 63 alone; a flat row and an all-zero row go with them.  A mean that is off shifts the whole row, which the window
spreads over the lowest depth bins of the LINEAR image (the DC mask touches the dB image only).

Waves take rows from a workgroup-wide ticket: 3 rows (fewer than waves) and 2 x 1030 = 2060 rows -- more than the 2048 waves
of a 256-CU launch, so workgroups claim beyond their first slots.  Every row of the 2060 must be there exactly once: each
output row is nearest to ITS oracle row among all 2060 (which are apart by far more than the tolerance).

Every case: helpers.check_mag / check_db against the oracle, both division settings, D x H = row-major and staged = fused
bit for bit.  One T = 32 plan and one T = 16 plan at their smallest shapes go through the same checks but the staged
comparison: they share the sums' helper, of which they take the shuffle branch."""
import functools

import numpy as np
import pytest

import helpers
from fdoct_amd import LAYOUT_TRANSPOSED, Config, Reconstructor, synth

pytestmark = pytest.mark.gpu

W = N = 2048
D = 1024
FLAT = 30000          # camera counts of the flat level
SPL = 8               # samples per lane and quarter row
QUARTER = 64 * SPL    # a chunk: 64 lanes x 8 samples


def _lane_samples(lanes, quarters=(0, 1, 2, 3)):
    """Sample indices that the given lanes own in the given quarters of the row."""
    return np.concatenate([np.arange(SPL * l, SPL * l + SPL) + QUARTER * q for q in quarters for l in lanes])


def _deviation(idx):
    """What the samples idx carry instead of the flat level: a step and a fringe, so that the row's mean, its reference sample
    and its spectrum all depend on them."""
    return np.rint(FLAT + 2500.0 + 1800.0 * np.cos(0.37 * idx)).astype(np.uint16)


SUM_ROWS = (
    [("group %d" % g, _lane_samples(range(16 * g, 16 * g + 16))) for g in range(4)]
    + [("lanes 15/16", _lane_samples((15, 16))), ("lanes 31/32", _lane_samples((31, 32))),
       ("lanes 47/48", _lane_samples((47, 48))), ("lane 63", _lane_samples((63,))),
       ("flat", np.arange(0)), ("zero", None)]
)


@functools.lru_cache(maxsize=None)
def _sum_rows_case():
    """One frame whose rows are SUM_ROWS, the background, and the oracle's (linear, dB in (G, H, D))."""
    frame = np.full((1, len(SUM_ROWS), W), FLAT, np.uint16)
    for r, (_, idx) in enumerate(SUM_ROWS):
        if idx is None:
            frame[0, r] = 0
        else:
            frame[0, r, idx] = _deviation(idx)
    return _with_oracle(frame, W, N, D)


@functools.lru_cache(maxsize=None)
def _synth_case(w, n, d, H, nframes):
    return _with_oracle(synth.make_frames(11, nframes, w, H), w, n, d)


def _with_oracle(frames, w, n, d):
    yb = synth.make_background(w)
    cfg = Config(width=w, height=frames.shape[1], numfftpoints=n, numdisplaypoints=d)
    mag, _, db = helpers.oracle_reference(cfg, frames, yb)
    db = np.ascontiguousarray(np.transpose(db, (0, 2, 1)))
    for a in (frames, yb, mag, db):
        a.setflags(write=False)
    return cfg, frames, yb, mag, db


def _run_and_check(case, what, plan=None, staged=True):
    """Both division settings; D x H and the staged chain bit for bit; the oracle.  Returns the two linear images."""
    cfg, frames, yb, mag_o, db_o = case
    out = []
    for precise in (True, False):
        w = "%s, %s division" % (what, "two-word" if precise else "one-word")
        r = Reconstructor(cfg)
        r.set_background(yb)
        r.set_precise_division(precise)
        if plan is not None:
            r.set_plan(plan, False)
        b, d = r.process(frames)
        bt, dt = r.process(frames, layout=LAYOUT_TRANSPOSED)
        if staged:
            r.set_staged(True)
            bs, ds = r.process(frames)
        r.close()
        np.testing.assert_array_equal(bt, np.transpose(b, (0, 2, 1)), w + ": D x H linear")
        np.testing.assert_array_equal(dt, np.transpose(d, (0, 2, 1)), w + ": D x H dB")
        if staged:
            np.testing.assert_array_equal(bs, b, w + ": staged linear")
            np.testing.assert_array_equal(ds, d, w + ": staged dB")
        w_mag = helpers.check_mag(b, mag_o, w)
        w_db = helpers.check_db(d, db_o, mag_o, w)
        print("%s: err/tol linear %.3f dB %.3f" % (w, w_mag, w_db))
        out.append(b)
    return out


def test_sums_on_rows_confined_to_lane_groups_and_group_edges():
    cfg, frames, yb, mag_o, db_o = case = _sum_rows_case()
    # the rows are what they are meant to be: flat outside the named lanes' samples, and the oracle tells them apart
    for r, (name, idx) in enumerate(SUM_ROWS):
        others = np.ones(W, bool)
        if idx is not None:
            others[idx] = False
            assert (frames[0, r, others] == FLAT).all(), name
            assert idx.size == 0 or (frames[0, r, idx] != FLAT).any(), name
    assert np.isfinite(mag_o).all() and np.isfinite(db_o).all()
    assert (mag_o[0, -1] == mag_o[0, -1, 0]).all(), "the oracle's all-zero row: epsilon in every bin"
    for b in _run_and_check(case, "sum rows"):
        # row by row, so that a failure names the row (check_mag above has already held the whole image to the tolerance)
        for r, (name, _) in enumerate(SUM_ROWS):
            worst = float(helpers.mag_ratio(b[:, r:r + 1], mag_o[:, r:r + 1]).max())
            assert worst <= 1.0, "row '%s': worst linear error/tolerance %.3g" % (name, worst)
        assert (b[0, -1] == b[0, -1, 0]).all(), "the all-zero row: one value in every bin"


def test_three_rows():
    _run_and_check(_synth_case(W, N, D, 3, 1), "3 rows")


def test_2060_rows_each_present_exactly_once():
    H, nframes = 1030, 2
    case = _synth_case(W, N, D, H, nframes)
    o = case[3].reshape(nframes * H, D).astype(np.float64)
    sq_o = (o * o).sum(axis=1)

    def distances(x):   # (rows of x) x (rows of the oracle), Euclidean
        return np.sqrt(np.maximum((x * x).sum(axis=1)[:, None] + sq_o[None, :] - 2.0 * (x @ o.T), 0.0))

    # the oracle's rows are apart by far more than the tolerance lets a row move
    tol = helpers.RTOL * np.abs(o) + helpers.ATOL_ROWMAX * np.abs(o).max(axis=1, keepdims=True)
    apart = distances(o)
    np.fill_diagonal(apart, np.inf)
    assert apart.min() > 10.0 * np.sqrt((tol * tol).sum(axis=1)).max(), "the oracle's rows are too alike to tell a misplaced row"
    for b in _run_and_check(case, "2060 rows"):
        nearest = distances(b.reshape(nframes * H, D).astype(np.float64)).argmin(axis=1)
        np.testing.assert_array_equal(nearest, np.arange(nframes * H), "every row once, in its place")


@pytest.mark.parametrize("name, w, n, d, plan, staged", [("T = 32: the 32 x 32 plan on half waves", 2048, 2048, 1024, 3, False),
                                                          ("T = 16: the 256-point plan", 512, 512, 256, None, False)],
                         ids=["T32", "T16"])
def test_plans_with_shorter_lane_groups(name, w, n, d, plan, staged):
    _run_and_check(_synth_case(w, n, d, 3, 1), name, plan=plan, staged=staged)
