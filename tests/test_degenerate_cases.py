"""CPU checks of tests/degenerate_cases.py, for every case tests/test_gpu_degenerate_inputs.py runs: every row is what its name
says; the oracle's linear and dB images are finite; its empty rows are exactly the ones degenerate_cases.empty_rows names and
equal epsilon in every bin; the rows that are not empty differ pairwise by more than their tolerance (a kernel that serves one
row's result for another fails); and the f32 restatement lies within helpers.TRUTH_LIMIT of the chain in double -- the reference
alone stays inside the rule, so max(TRUTH_LIMIT, the oracle's own distance) never widens what the GPU is allowed."""
import numpy as np
import pytest

import chain_grid_sizes as grids
import degenerate_cases as dg
import helpers


@pytest.mark.parametrize("top", [65535, 255])
@pytest.mark.parametrize("W", [160, 1024])
def test_rows_are_what_they_are_called(W, top):
    for kind in ("clean", "dead", "full"):
        yb = dg.background(kind, W, dg.ROWS, top)
        assert np.array_equal(yb, np.rint(yb)) and yb.min() >= 0 and yb.max() <= top
        dead = dg.dead_columns(W)
        if kind == "clean":
            assert yb.shape == (W,) and yb.min() > 0
        else:
            rows2d = np.atleast_2d(yb)
            assert (rows2d[:, dead] == 0).all()
            if kind == "full":
                assert yb.shape == (dg.ROWS, W) and (yb[dg.BLOCKED_ROW] == 0).all() and dg.BLOCKED_ROW == dg.ORDINARY_2
                rows2d = np.delete(rows2d, dg.BLOCKED_ROW, axis=0)
                assert len({tuple(r) for r in rows2d}) == dg.ROWS - 1       # every row scaled on its own
            assert (rows2d[:, dg.ONE_COLUMN] == 1).all() and (np.delete(rows2d, dead, axis=1) > 0).all()
        yb_row = yb[dg.NO_FRINGE] if yb.ndim == 2 else yb
        f = dg.frame_rows(W, yb_row, top)
        assert f.shape == (dg.ROWS, W) and f.dtype == (np.uint8 if top == 255 else np.uint16) and dg.ROWS % 4 != 0
        assert (f[dg.ZEROS] == 0).all() and (f[dg.TOP] == top).all()
        assert (f[dg.MID] == f[dg.MID, 0]).all() and 0 < f[dg.MID, 0] < top
        assert np.array_equal(f[dg.NO_FRINGE].astype(np.float64), yb_row)     # the quotient is exactly 1 wherever the background is non-zero
        for r, c in ((dg.IMPULSE_LEFT, 1), (dg.IMPULSE_RIGHT, W - 2), (dg.IMPULSE_DEAD, W // 2)):
            assert f[r, c] == top and f[r].astype(np.int64).sum() == top
        assert (yb_row[W // 2] == 0) == (kind != "clean") and yb_row[1] > 1 and yb_row[W - 2] > 1
        assert (f[dg.ALTERNATING, 0::2] == 0).all() and (f[dg.ALTERNATING, 1::2] == top).all()
        assert np.array_equal(f[dg.COPY], f[dg.ORDINARY]) and not np.array_equal(f[dg.ORDINARY_2], f[dg.ORDINARY])
        for r in (dg.ORDINARY, dg.ORDINARY_2):                                # ordinary: fringes over a positive level
            assert f[r].min() >= 0 and f[r].max() > f[r].mean() * 1.5 and len(np.unique(f[r])) > W // 8
        tall = dg.frame_rows(W, yb_row, top, 20)
        assert np.array_equal(tall[:dg.ROWS], f) and np.array_equal(tall[dg.ROWS:], dg.ordinary_rows(W, 20, top)[dg.ROWS:])
    H = dg.ROWS
    c = dg.constant_frame(W, H, top)
    assert c.min() == c.max() == dg.mid_value(top)
    k = dg.corners_frame(W, H, top)
    assert np.flatnonzero(k == 0).tolist() == [0] and np.flatnonzero(k == top).tolist() == [H * W - 1]
    f = dg.frame_rows(W, dg.background("clean", W, H, top), top)
    yd = dg.dark_frame(f, top)
    diff = f[0::2] - yd[0::2]
    assert (diff <= 0).all() and (diff < 0).mean() > 0.99                    # negative after the subtraction
    assert (yd[1::2] <= 0.02 * top).all() and np.array_equal(yd[dg.COPY], yd[dg.ORDINARY])
    assert np.array_equal(dg.pi_frame(f), f)


def test_families_and_their_cases():
    assert len(set(dg.FAMILY_IDS)) == len(dg.FAMILIES)
    for fam in dg.FAMILIES:
        g = fam.geometry
        assert fam.H in (dg.ROWS, 20) and len(set(fam.cases)) == len(fam.cases)
        assert (fam.H == 20) == (fam.layout == dg.DXH)                 # 20 rows close the transposed store's tiles
        for case in fam.cases:
            i = dg.inputs(fam.name, case)
            assert i.frames.shape == (i.cfg.averages, fam.H, g["width"])
            assert i.frames.dtype == (np.uint8 if case.bits == 8 else np.uint16)
            assert (i.yb.max() <= 1.0) == (case.opt != "plain")
            assert i.yb.shape == ((fam.H, g["width"]) if case.bg == "full" else (g["width"],))
            if case.frames == "pair":
                assert not i.frames[1].any()
    W, M, N, D = (dg.family("workgroup-per-row, 1024 threads, 2400 x 4").geometry[k] for k in
                  ("width", "increasefftpointsmultiplier", "numfftpoints", "numdisplaypoints"))
    assert grids.generic_threads(grids.generic_lds(W, M, N, D)) == 1024
    W, M, N, D = (dg.family("workgroup-per-row, 2048 -> 2002").geometry[k] for k in
                  ("width", "increasefftpointsmultiplier", "numfftpoints", "numdisplaypoints"))
    assert grids.generic_threads(grids.generic_lds(W, M, N, D)) == 256


def _pairs_apart(truth_rows):
    """The smallest over all pairs of rows of max_bins |a - b| / (tol(a) + tol(b))."""
    tol = helpers.RTOL * np.abs(truth_rows) + helpers.ATOL_ROWMAX * np.abs(truth_rows).max(axis=-1, keepdims=True)
    worst = np.inf
    for a in range(len(truth_rows)):
        for b in range(a + 1, len(truth_rows)):
            worst = min(worst, float((np.abs(truth_rows[a] - truth_rows[b]) / (tol[a] + tol[b])).max()))
    return worst


@pytest.mark.parametrize("name", dg.FAMILY_IDS)
def test_oracle_on_every_case(name):
    fam = dg.family(name)
    for case in fam.cases:
        what = "%s, %s" % (name, case)
        mag_o, db_o, mag_t, db_t = dg.reference(name, case)
        assert mag_o.shape == (1, fam.H, fam.geometry["numdisplaypoints"]) == db_o.shape == mag_t.shape == db_t.shape
        for a in (mag_o, db_o, mag_t, db_t):
            assert np.isfinite(a).all(), what
        eps = dg.eps_of(case)
        want = dg.empty_rows(case, fam.H)
        for m in (mag_o, mag_t):
            assert np.flatnonzero(dg.is_empty(m[0], eps)).tolist() == want, what
            assert (m[0] >= eps).all()
        assert set(dg.dc_level_rows(case)) <= set(want)
        # (the rows that hold zeros before any rounding are exactly epsilon in double too)
        exact = dg.exact_empty_rows(case, fam.H)
        assert set(want) - set(exact) <= {dg.NO_FRINGE}
        assert (mag_t[0, exact] == eps).all() and (mag_o[0, exact] == eps).all(), what
        rows = dg.distinct_rows(case)
        if rows:
            assert _pairs_apart(mag_t[0, rows]) > 1.0, what
        g, o = helpers.truth_ratios(mag_o, mag_t, mag_o)
        assert g == o and o <= helpers.TRUTH_LIMIT, "%s: the f32 restatement is %.3g x the tolerance from the chain in double" % (what, o)
        od = float(helpers.db_ratio(db_o, db_t, mag_t).max())
        assert od <= helpers.TRUTH_LIMIT, "%s: dB, %.3g" % (what, od)


def test_half_float_pattern_stays_inside_the_fallback_bound():
    """The families whose second word of 1/background is the half-float pattern: what that form leaves of the no-fringe row
    (degenerate_cases.half_pattern_no_fringe_row) is more than the 1e-9 the rule allows a row of pure epsilon, and far inside
    SURVEY 8(d)'s tolerance at the peak of the frame's ordinary row 0 -- the bound those families are held to on that row."""
    assert set(dg.HALF_PATTERN) <= set(dg.FAMILY_IDS)
    seen = 0
    for name in dg.HALF_PATTERN:
        for case in dg.family(name).cases:
            if not (dg.half_pattern(name, case) and dg.NO_FRINGE in dg.dc_level_rows(case)):
                continue
            seen += 1
            _, _, mag_t, _ = dg.reference(name, case)
            row = dg.half_pattern_no_fringe_row(name, case)
            truth = mag_t[0, dg.NO_FRINGE]
            left = float(np.abs(row - truth).max())
            assert 2e-11 < left < 2.0 ** -35 * 6 * mag_t.shape[-1], (name, case, left)      # (at most 6 x 2^-35 per sample of the row: a, b and the mean)
            g = helpers.truth_ratios(row[None], truth[None], rowmax=np.abs(mag_t[0, dg.ORDINARY]).max())[0]
            assert g <= 1e-3 * helpers.TRUTH_LIMIT, (name, case, g)
    assert seen >= 6
