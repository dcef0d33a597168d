"""CPU checks of tests/doppler_edge_cases.py from tests/doppler_model.py alone, as tests/test_doppler_cases.py checks the first 17
cases: every seam case and every window of the sweep keeps its exemptions under 1 % of its bins, is passed by the float composition
itself, stays under the recorded arctan2 figure and keeps |B| >= 16 tol_B where the bulk correction is on; the reach of a sample
is what doppler_model.brute shows for the same NaN; the LDS-byte formula puts 65 520 and 65 940 bytes on the two sides of 64 KiB;
the tall batch's sizes hold their conditions for several CU counts; the exact field gives exact outputs in the float
composition; and the tables cannot silently shrink."""
import numpy as np
import pytest

import doppler_cases as dc
import doppler_edge_cases as de
import doppler_model as dm


def _conditions(X, kw, what):
    geo = dict(axis=kw["axis"], lag=kw["lag"], win=kw["win"], bulk=kw["bulk"])
    ill, edge = dm.exemptions(X, min_power=kw["min_power"], **geo)
    assert ill.sum() <= 0.01 * ill.size and edge.sum() <= 0.01 * edge.size, "%s: %d + %d of %d bins exempt" % (what, ill.sum(), edge.sum(), ill.size)
    tol = dm.tolerances(X, **geo)
    fl, tr = dm.model(X, **kw), dm.model(X, truth=True, **kw)
    if kw["bulk"]:
        assert np.all(tol["tol_B"] > 0), what
        assert np.all(np.abs(tol["B"]) >= 16 * tol["tol_B"]), what + ": |B| < 16 tol_B"
        assert dm._ratio(fl["B"], tol["B"], tol["tol_B"]) <= 1.0, what
    rR, rP = dm._ratio(fl["corr"], tr["corr"], tol["tol_R"]), dm._ratio(fl["power"], tr["power"], tol["tol_P"])
    assert rR <= 1.0 and rP <= 1.0, "%s: the float composition's own ratios: corr %.4f, power %.4f" % (what, rR, rP)
    R = fl["corr"]
    a32 = np.arctan2(R.imag, R.real)
    assert a32.dtype == np.float32
    worst = float(np.abs(dm.wrap(a32.astype(np.float64) - np.arctan2(R.imag.astype(np.float64), R.real.astype(np.float64)))).max())
    assert worst <= dm.ATAN2F_HOST, "%s: |float32 arctan2 - float64 arctan2| = %.3g rad" % (what, worst)
    print("%s: %d bins exempt, own ratios corr %.4f power %.4f, arctan2 %.3g rad" % (what, ill.sum() + edge.sum(), rR, rP, worst))
    return int(ill.sum() + edge.sum()), rR, rP, worst


@pytest.mark.parametrize("case", de.SEAM_CASES + de.SEAM_BULK_CASES, ids=[c["what"] for c in de.SEAM_CASES + de.SEAM_BULK_CASES])
def test_every_seam_case_keeps_its_conditions(case):
    _conditions(dc.case_field(case), dc.case_args(case), case["what"])


@pytest.mark.parametrize("group", list(de.WINDOW_GROUPS))
def test_every_window_of_the_sweep_keeps_its_conditions(group):
    X = de.sweep_field()
    for win in de.WINDOW_GROUPS[group]:
        _conditions(X, de.sweep_args(win), "%d x %d on %d x %d x %d" % (win + de.SWEEP_SHAPE))


def test_case_lists_cover_what_the_gpu_tests_are_asked_for():
    assert len(de.SEAM_CASES) == 36 and len(de.SEAM_BULK_CASES) == 12
    pair = lambda c: dm.pair_shape(c["axis"], c["lag"], c["n"], c["H"])[1]   # noqa: E731
    assert {(pair(c), c["D"]) for c in de.SEAM_CASES} == {(r, d) for r in (15, 16, 17, 31, 32, 33) for d in (63, 64, 65, 127, 128, 129)}
    assert all(c["win"] == (4, 8) and c["axis"] == dm.ASCANS and c["lag"] == 1 and c["n"] == 2 and not c["bulk"] for c in de.SEAM_CASES)
    assert {pair(c) for c in de.SEAM_BULK_CASES} == set(de.SEAM_ROWS) and {c["D"] for c in de.SEAM_BULK_CASES} == set(de.SEAM_DEPTHS)
    assert len({(pair(c), c["D"]) for c in de.SEAM_BULK_CASES}) == 12
    assert all(c["win"] == (3, 5) and c["axis"] == dm.FRAMES and c["lag"] == 1 and c["n"] == 2 and c["bulk"] is True for c in de.SEAM_BULK_CASES)
    assert len({c["seed"] for c in de.SEAM_CASES + de.SEAM_BULK_CASES}) == 48
    # the sweep: 98 launches; every size 1 .. 32 on each axis alone, every size paired with its complement, the odd and even squares
    wins = [w for g in de.WINDOW_GROUPS.values() for w in g]
    assert len(wins) == 98 and all(1 <= a <= dc.MAX_WIN and 1 <= d <= dc.MAX_WIN for a, d in wins)
    assert {(w, 1) for w in range(2, 33)} | {(1, w) for w in range(2, 33)} | {(w, 33 - w) for w in range(1, 33)} <= set(wins)
    assert {(2, 2), (31, 31), (20, 29), (20, 30)} <= set(wins)
    assert de.WINDOW_GROUPS["either side of 64 KiB of LDS"] == list(de.LDS_STRADDLE)
    pr, D = de.SWEEP_SHAPE[1] - 1, de.SWEEP_SHAPE[2]
    assert dc.TILE_ROWS < pr < 2 * dc.TILE_ROWS and dc.TILE_DEPTHS < D < 2 * dc.TILE_DEPTHS
    # reach: both axes, both lags, an even and the 1 x 1 window, six positions each, the seam's four corners among them
    assert len(de.reach_configs()) == 8
    for axis, lag, win in de.reach_configs():
        pos = de.reach_positions(axis, lag)
        assert len(pos) == 6 and {(r, b) for _, r, b in pos[:4]} == {(15, 63), (15, 64), (16, 63), (16, 64)}
        n = de.reach_frames(axis, lag)
        assert pos[4] == (0, 0, 0) and pos[5] == (n - 1, de.REACH_H - 1, de.REACH_D - 1)
        pi, prr = dm.pair_shape(axis, lag, n, de.REACH_H)
        assert len(de.partners(axis, lag, pos[0], pi, prr)) == 2 and len(de.partners(axis, lag, pos[4], pi, prr)) == 1
        assert len(de.partners(axis, lag, pos[5], pi, prr)) == 1
    assert set(de.EXACT_WINDOWS) == {(1, 1), (2, 2), (3, 5), (4, 8)}


def test_the_lds_formula_straddles_64_kib():
    assert (dc.TILE_ROWS, dc.TILE_DEPTHS) == (16, 64)
    for wa in range(1, 33):
        for wd in range(1, 33):
            assert de.lds_bytes(wa, wd) == 12 * (15 + wa) * (127 + wd)
    below, above = (de.lds_bytes(*w) for w in de.LDS_STRADDLE)
    assert (below, above) == (65520, 65940) and below < de.LDS_DEFAULT_LIMIT == 65536 < above
    assert de.lds_bytes(32, 32) > de.LDS_DEFAULT_LIMIT and de.lds_bytes(1, 1) == 24576
    # the sweep's windows lie on both sides of the limit in every group but the one along depth, which stays below it
    for name, group in de.WINDOW_GROUPS.items():
        sides = {de.lds_bytes(*w) > de.LDS_DEFAULT_LIMIT for w in group}
        assert sides == ({False} if name == "along depth" else {False, True}), name
    assert de.lds_bytes(27, 1) <= de.LDS_DEFAULT_LIMIT < de.lds_bytes(28, 1)


# ---- reach ---------------------------------------------------------------------------------------------------------------------------
def test_reach_is_the_window_turned_round():
    """reach() states the outputs from the sample's side; the definition states the window from the output's side."""
    shape = (3, 9, 11)
    for axis in (dm.ASCANS, dm.FRAMES):
        for lag in (1, 2):
            pi, pr = dm.pair_shape(axis, lag, shape[0], shape[1])
            for win in ((1, 1), (2, 3), (4, 8), (5, 2), (32, 32)):
                for pos in ((0, 0, 0), (1, 4, 5), (2, 8, 10), (2, 1, 0)):
                    want = np.zeros((pi, pr, shape[2]), bool)
                    for p, q in de.partners(axis, lag, pos, pi, pr):
                        for r in range(pr):
                            for b in range(shape[2]):
                                if r - (win[0] - 1) // 2 <= q <= r + win[0] // 2 and b - (win[1] - 1) // 2 <= pos[2] <= b + win[1] // 2:
                                    want[p, r, b] = True
                    assert np.array_equal(de.reach(axis, lag, win, pos, shape), want), (axis, lag, win, pos)
                    assert np.array_equal(de.reach(axis, lag, win, pos, shape, all_depths=True), want.any(-1, keepdims=True) & np.ones(want.shape, bool))


def _nan(a):
    return np.isnan(a.real) | np.isnan(a.imag)


@pytest.mark.parametrize("cfg", de.reach_configs(), ids=lambda c: "axis %d, lag %d, %d x %d" % (c[0], c[1], c[2][0], c[2][1]))
def test_reach_is_where_the_definition_turns_nan(cfg):
    """doppler_model.brute on the field with one sample NaN: R and P are NaN exactly in the sample's reach and keep their bits
    outside it; with the bulk correction, every row out of reach of the sample's pair rows keeps its bits."""
    axis, lag, win = cfg
    X = de.reach_field(axis, lag)
    R0, P0, _ = dm.brute(X, axis, lag, win)
    Rb0, _, _ = dm.brute(X, axis, lag, win, bulk=True)
    for pos in de.reach_positions(axis, lag):
        Y = de.poisoned(X, pos)
        R, P, _ = dm.brute(Y, axis, lag, win)
        hit = de.reach(axis, lag, win, pos, X.shape)
        assert hit.any() and not hit.all()
        assert np.array_equal(_nan(R), hit) and np.array_equal(np.isnan(P), hit), (cfg, pos)
        assert np.array_equal(R[~hit], R0[~hit]) and np.array_equal(P[~hit], P0[~hit]), (cfg, pos)
        Rb, _, _ = dm.brute(Y, axis, lag, win, bulk=True)
        rows = de.reach(axis, lag, win, pos, X.shape, all_depths=True)
        assert np.array_equal(Rb[~rows], Rb0[~rows]) and np.array_equal(_nan(Rb) & ~rows, np.zeros(rows.shape, bool)), (cfg, pos)


# ---- the tall batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [16, 64, 104, 228, 256, 304])
@pytest.mark.parametrize("axis", [dm.ASCANS, dm.FRAMES])
def test_tall_batch_sizes(axis, cus):
    n = de.tall2_frames(axis, cus)
    assert de.tall2_ok(axis, n, cus) and n % 3 == 0
    pi, pr = de.tall2_shape(axis, n)
    assert -(-pr // dc.TILE_ROWS) == 2 and -(-de.TALL2_D // dc.TILE_DEPTHS) == 2       # two tiles each way a pair image
    t = dc.tiles(pi, pr, de.TALL2_D)
    assert t == 4 * pi and t >= 1.5 * dc.grid_cap(cus) and t % dc.grid_cap(cus) != 0
    if de.TALL2_BULK[axis]:
        assert pi * pr >= 1.5 * dc.grid_cap(cus) and (pi * pr) % dc.grid_cap(cus) != 0
    assert de.tall2_base_ok(axis, cus)
    assert n * de.TALL2_H * de.TALL2_D * 8 < 8 << 20   # the tall batch stays small
    if cus == 256:
        assert 380 <= n <= 400


def test_one_axis_of_the_tall_batch_runs_the_bulk_kernel():
    assert sorted(map(bool, de.TALL2_BULK.values())) == [False, True] and de.TALL2_WIN == (4, 8)
    assert de.TALL2_BASE == {dm.ASCANS: (3, 1), dm.FRAMES: (6, 3)}


# ---- the exact field -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", de.EXACT_WINDOWS, ids=lambda w: "%d x %d" % w)
def test_the_exact_field_is_exact_in_the_float_composition(win):
    X = de.exact_field()
    assert X.dtype == np.complex64 and X.shape == de.SWEEP_SHAPE
    edge = float(np.nextafter(np.float32(de.EXACT_POWER), np.float32(np.inf)))
    assert edge > de.EXACT_POWER and float(np.float32(edge)) == edge
    cnt = dm.count(X.shape[1] - 1, X.shape[2], *win)
    for truth in (False, True):
        m = dm.model(X, dm.ASCANS, 1, win, min_power=de.EXACT_POWER, truth=truth)
        assert np.all(m["power"] == de.EXACT_POWER) and np.all(m["corr"].real == 0) and np.all(m["corr"].imag == de.EXACT_POWER * cnt)
        assert np.all(np.abs(m["phase"].astype(np.float64) - np.pi / 2) <= dm.PHASE_TOL)         # at the threshold: not masked
        m = dm.model(X, dm.ASCANS, 1, win, min_power=edge, truth=truth)
        assert np.all(m["phase"] == 0) and np.all(m["power"] == de.EXACT_POWER)                    # one ulp above it: all masked
    assert np.all(dm.model(X, dm.ASCANS, 1, win)["phase"] == np.float32(np.pi / 2))


# ---- behind the chain ----------------------------------------------------------------------------------------------------------------
def test_the_chain_cases_meet_both_axes_and_both_bulk_settings():
    import complex_cases as cc
    assert len(cc.OPTION_CASES) == 2 * len(cc.KINDS) + 1
    for kind in cc.KINDS + (cc.FOUR_BITS,):
        met = [ab for c in cc.OPTION_CASES if c.kind == kind for ab in de.option_axes(c)]
        assert {a for a, _ in met} == {dm.ASCANS, dm.FRAMES} and {bool(b) for _, b in met} == {False, True}, kind
    assert sorted((c.route, c.D) for c in de.chain_depth_cases()) == sorted((r, D) for r in ("wave", "generic") for D in (1, 63, 64, 65))
