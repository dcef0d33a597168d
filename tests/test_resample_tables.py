"""CPU checks of tests/resample_tables.py, for every (family, table) pair tests/test_gpu_resample_tables.py runs: every table is
legal for fdoct_set_resample_table; the tables the library builds itself never gather sample 0 or the last samples and walk
monotonically -- the gap the custom tables exist for, asserted so that a change of the builder says the premise changed; every
custom table does what its name says; and under every table the oracle stays finite, its f32 restatement lies within
resample_tables.ORACLE_LIMIT = 0.25 of the tolerance of the chain in double (a condition on the inputs: half of
helpers.TRUTH_LIMIT, so the reference alone never widens what the GPU is allowed), and the two ordinary rows differ by more than
their tolerance.  The oracle's statement of slopes[0] = slopes[1] (main:1161) is written out against its data_ylin."""
import numpy as np
import pytest

import degenerate_cases as dg
import helpers
import oracle_lib as orc
import resample_tables as rt


def _steps(idx):
    return np.diff(rt.gathered(idx).astype(np.int64))


def test_families_and_their_tables():
    assert len(set(rt.FAMILY_IDS)) == len(rt.FAMILIES) and set(dg.FAMILY_IDS) <= set(rt.FAMILY_IDS)
    assert set(rt.SETTER_FAMILIES) <= set(rt.FAMILY_IDS)
    for fam in rt.FAMILIES:
        W, M, N, D = rt.shape(fam)
        i = rt.inputs(fam.name)
        assert i.frames.shape == (1, fam.H, W) and i.frames.dtype == (np.uint8 if fam.bits == 8 else np.uint16)
        assert i.yb.shape == (W,) and i.yb.min() > 0 and i.cfg.averages == 1
        assert (i.phase is not None) == fam.phase and (i.phase is None or i.phase.shape == (N, 2))
        assert tuple(fam.tables) == (rt.LONG_TABLES if fam.name.startswith("long rows") else rt.TABLES)
        assert not np.array_equal(i.frames[0, dg.ORDINARY], i.frames[0, dg.ORDINARY_2])
    W, M, N, _ = rt.shape(rt.family("workgroup-per-row, full-length zero-pad, 161 x 4"))
    assert W % 2 == 1 and M % 2 == 0 and W + 2 * ((M * W - W) // 2) == M * W - 1      # column M W - 1 does not exist (main:229)
    W, M, N, _ = rt.shape(rt.family("wave-per-row, 1280 x 4 -> 2560"))
    assert M * W > N                                                                  # fractionalk is indexed past its end


@pytest.mark.parametrize("name", rt.FAMILY_IDS)
def test_every_table_is_legal_and_what_it_is_called(name):
    fam = rt.family(name)
    W, M, N, _ = rt.shape(fam)
    MW = M * W
    cfg = rt.inputs(name).cfg
    idx0, frac0 = rt.default_table(W, M, N, cfg.lambdamin, cfg.lambdamax)
    # the premise: what the built tables never reach
    for idx_d in (idx0, rt.family_table(name, "wide")[0]) if "wide" in fam.tables else (idx0,):
        g = rt.gathered(idx_d)
        assert g.min() >= 1, "the built table gathers sample 0: the premise of these tests changed"
        assert g.max() <= MW - 2, "the built table gathers the last sample: the premise of these tests changed"
        assert (_steps(idx_d) <= 0).all(), "the built table is not monotone: the premise of these tests changed"
    f0 = frac0[rt.gathered(idx0)[rt.gathered(idx0) < N]]
    assert (f0 > 0).all() and (f0 <= 1).all()
    for t in fam.tables:
        idx, frac = rt.family_table(name, t)
        assert idx.shape == (N,) and idx.dtype == np.int32 and frac.shape == (N,) and frac.dtype == np.float64, t
        assert idx.min() >= 0 and idx.max() < MW and np.isfinite(frac).all(), t
        again = rt.table(t, W, M, N, cfg.lambdamin, cfg.lambdamax)
        assert np.array_equal(again[0], idx) and np.array_equal(again[1], frac), t      # deterministic
        g, s = rt.gathered(idx), _steps(idx)
        if t.startswith("ends"):
            assert g[0] == 0 and g[-1] == MW - 1 and (s >= 0).all() and frac[0] == rt.FRAC_AT_0 != 0
            assert MW - 1 >= N or frac[MW - 1] == rt.FRAC_AT_LAST
        elif t in ("reversed", "evenodd", "sawtooth"):
            assert (s > 0).any(), t                                                     # not the built tables' walk down the row
            if t == "reversed":
                assert (s >= 0).all() and np.array_equal(idx, idx0[::-1])
            else:
                assert (s < 0).any(), t
            if t == "evenodd":
                assert s.max() > (g.max() - g.min()) * 0.9                              # one jump back across the gathered span
            if t == "sawtooth":
                assert (s < -MW // 2).sum() == 3 and g.min() == 0 and g.max() >= MW - 1 - (4 * MW + N - 1) // N   # four ramps
        elif t == "held":
            runs = idx[:N - N % rt.HELD].reshape(-1, rt.HELD)
            assert (runs == runs[:, :1]).all() and len(np.unique(runs[:, 0])) > 1
        elif t == "extrapolating":
            f = frac[g[g < N]]
            assert f.min() < 0 and f.max() > 1 and f.min() >= -0.5 and f.max() <= 1.5 and np.array_equal(idx, idx0)
        if t == "ends+hamming":
            w = rt.window(t, W)
            assert np.array_equal(idx, rt.family_table(name, "ends")[0]) and np.array_equal(frac, rt.family_table(name, "ends")[1])
            assert w.shape == (W,) and abs(w[0] - 0.08) < 1e-12 and abs(w[-1] - 0.08) < 1e-12 and rt.window("ends", W) is None
            continue
        if t != "extrapolating" and t != "ends":
            assert np.array_equal(frac, rt.default_table(W, M, N, *rt.WIDE_RANGE)[1] if t == "wide" else frac0), t


def _apart(a, b):
    """max over the bins of |a - b| / (tol(a) + tol(b)) for two truth rows."""
    ta = helpers.RTOL * np.abs(a) + helpers.ATOL_ROWMAX * np.abs(a).max()
    tb = helpers.RTOL * np.abs(b) + helpers.ATOL_ROWMAX * np.abs(b).max()
    return float((np.abs(a - b) / (ta + tb)).max())


@pytest.mark.parametrize("name", rt.FAMILY_IDS)
def test_oracle_under_every_table(name):
    fam = rt.family(name)
    D = rt.shape(fam)[3]
    worst = {}
    for t in fam.tables:
        what = "%s, %s" % (name, t)
        mag_o, db_o, mag_t, db_t = rt.reference(name, t)
        assert mag_o.shape == (1, fam.H, D) == db_o.shape == mag_t.shape == db_t.shape
        for a in (mag_o, db_o, mag_t, db_t):
            assert np.isfinite(a).all(), what
        g, o = helpers.truth_ratios(mag_o, mag_t, mag_o)
        od = float(helpers.db_ratio(db_o, db_t, mag_t).max())
        worst[t] = (round(o, 3), round(od, 3))
        assert g == o and o <= rt.ORACLE_LIMIT, "%s: the f32 restatement is %.3g x the tolerance from the chain in double" % (what, o)
        assert od <= helpers.TRUTH_LIMIT, "%s: dB, %.3g" % (what, od)
        assert _apart(mag_t[0, dg.ORDINARY], mag_t[0, dg.ORDINARY_2]) > 1.0, what
        assert np.array_equal(mag_t[0, dg.COPY], mag_t[0, dg.ORDINARY])
    print(name, worst)
    # the slope rule of sample 0 is there to be seen under the Hamming window, and is not under the built one
    seen, unseen = rt.slope_rule_weight(name, "ends+hamming"), rt.slope_rule_weight(name, "ends")
    print(name, "slopes[0] = slopes[1] is worth, in tolerances of a bin: Hamming", seen.round(1), "Bartlett-Hann", unseen.round(2))
    if name == "long rows, 2048 x 8":    # (a 65536-point row upsampled x 8: 1.7 x; the same kernel's branch is seen on 'rows in HBM, 161 x 4')
        assert rt.family("rows in HBM, 161 x 4").kernel == fam.kernel
    else:
        assert seen.max() > 10.0 and seen.min() > 2.0, (name, seen)
    # the tables differ from the built one in what the chain gives
    if "ends" in fam.tables and "reversed" in fam.tables:
        assert _apart(rt.reference(name, "ends")[2][0, dg.ORDINARY], rt.reference(name, "reversed")[2][0, dg.ORDINARY]) > 1.0


@pytest.mark.parametrize("name", ["fused fast path, 1024-point plan", "workgroup-per-row, full-length zero-pad, 161 x 4", "wave-per-row, 160 x 4"])
def test_the_oracle_states_the_slope_rule_of_sample_zero(name):
    """`ends` gathers sample 0 at q = 1: data_ylin[1] = y[0] + fractionalk[0] (y[1] - y[0]) -- slopes[0] = slopes[1], main:1161 --
    on the row as the chain forms it (quotient, mean removed, window, zero-pad upsampling), written out here in double.  The
    comparison allows the last-place difference of a contracted multiply-add; the general formula, with y[-1] taken as 0 or as
    the row's last sample, is far outside it."""
    fam = rt.family(name)
    W, M, N, D = rt.shape(fam)
    i = rt.inputs(name)
    idx, frac = rt.family_table(name, "ends")
    win = orc.barthann(W)
    p = orc.make_params(W, fam.H, N, D, M)
    _, ylin = orc.frame_to_mag(p, i.frames[0].astype(np.float64), i.yb, None, win, idx, frac, want_ylin=True)
    y = i.frames[0].astype(np.float64) / i.yb[None, :]
    mean = np.cumsum(y, axis=1)[:, -1] / W                    # (summed from the left, as the oracle does)
    y = (y - mean[:, None]) * win[None, :]
    if M > 1:
        y = orc.zeropadrowwise(y, M)
    rows = [dg.ORDINARY, dg.ORDINARY_2]
    want = y[rows, 0] + frac[0] * (y[rows, 1] - y[rows, 0])
    scale = np.abs(y[rows, :2]).max(axis=1)
    assert (np.abs(ylin[rows, 1] - want) <= 4 * np.finfo(np.float64).eps * scale).all(), (ylin[rows, 1], want)
    for other in (y[rows, 0] + frac[0] * y[rows, 0], y[rows, 0] + frac[0] * (y[rows, 0] - y[rows, -1])):
        assert (np.abs(ylin[rows, 1] - other) > 1e-6 * scale).all()
    assert (ylin[:, 0] == 0).all() and (ylin[:, N - 1] == 0).all()
    if name.startswith("workgroup-per-row, full-length"):    # the column that does not exist is 0: data_ylin[N-2] = -g y[MW-2]
        assert (y[:, M * W - 1] == 0).all()
        assert np.allclose(ylin[rows, N - 2], -rt.FRAC_AT_LAST * y[rows, M * W - 2], rtol=1e-14, atol=0)
