"""CPU tests of tests/doppler_model.py, the numpy specification of the Doppler stage (include/fdoct_doppler.h): both forms against
the definition written as a double loop, the 1 x 1 window against INTEGRATION 2i's numpy lines, a known phase ramp recovered, the
bulk correction removing a constant offset added to one A-scan, and the edge counts."""
import numpy as np
import pytest

import doppler_cases as dc
import doppler_model as dm

SMALL = [
    ("A-scans lag 1, 3 x 5", dm.ASCANS, 1, (3, 5), None),
    ("A-scans lag 2, 4 x 8 (even windows: one more term ahead than behind)", dm.ASCANS, 2, (4, 8), None),
    ("frames lag 1, 2 x 3, bulk", dm.FRAMES, 1, (2, 3), True),
    ("frames lag 2, 32 x 32 (beyond the image), bulk over a sub-range", dm.FRAMES, 2, (32, 32), (3, 9)),
    ("A-scans lag 8 (one pair row), 3 x 1", dm.ASCANS, 8, (3, 1), None),
]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_both_forms_against_the_double_loop(case):
    what, axis, lag, win, bulk = case
    X = dc.field(3, 9, 21, 40, speckle=True)
    R, P, cnt = dm.brute(X, axis, lag, win, bulk)
    tr = dm.model(X, axis, lag, win, bulk, truth=True)
    fl = dm.model(X, axis, lag, win, bulk)
    tol = dm.tolerances(X, axis, lag, win, bulk)
    assert fl["corr"].dtype == np.complex64 and fl["power"].dtype == fl["phase"].dtype == np.float32
    assert tr["corr"].shape == R.shape == (dm.pair_shape(axis, lag, 3, 9) + (21,))
    np.testing.assert_array_equal(tr["cnt"], cnt)
    scale = np.abs(R).max()
    assert np.abs(tr["corr"] - R).max() <= 1e-12 * scale and np.abs(tr["power"] - P).max() <= 1e-12 * P.max()   # (another order of the same double sums)
    assert dm._ratio(fl["corr"], R, tol["tol_R"]) <= 1.0 and dm._ratio(fl["power"], P, tol["tol_P"]) <= 1.0
    np.testing.assert_allclose(tr["phase"], np.angle(R), atol=1e-9)


def test_one_by_one_window_is_the_numpy_lines_of_the_integration_guide():
    X = dc.field(2, 7, 33, 41)
    got = dm.model(X, dm.ASCANS, 1)
    want = np.angle(X[:, 1:].astype(np.complex128) * np.conj(X[:, :-1].astype(np.complex128)))
    assert np.abs(dm.wrap(got["phase"] - want)).max() <= 1e-5   # float products against double ones, on pairs well above the noise
    tr = dm.model(X, dm.ASCANS, 1, truth=True)
    np.testing.assert_allclose(tr["phase"], want, atol=1e-12)
    assert np.all(tr["cnt"] == 1)
    # ... and the magnitude mask of those lines is min_power on (|X1|^2 + |X2|^2) / 2
    p = (np.abs(X[:, 1:].astype(np.complex128)) ** 2 + np.abs(X[:, :-1].astype(np.complex128)) ** 2) / 2
    m = float(np.float32(np.median(p)))
    masked = dm.model(X, dm.ASCANS, 1, min_power=m, truth=True)["phase"]
    np.testing.assert_array_equal(masked, np.where(p < m, 0, want))


@pytest.mark.parametrize("axis", [dm.ASCANS, dm.FRAMES])
def test_a_known_phase_ramp_is_recovered(axis):
    n, H, D, w = 5, 9, 16, 0.37
    k = (np.arange(n)[:, None, None] if axis == dm.FRAMES else np.arange(H)[None, :, None]) * np.ones((n, H, D))
    amp = np.random.default_rng(3).uniform(1.0, 2.0, (n, H, D))
    X = (amp * np.exp(1j * w * k)).astype(np.complex64)
    for lag in (1, 2):
        for truth in (False, True):
            out = dm.model(X, axis, lag, (3, 5), scale=2.0, truth=truth)
            assert np.abs(out["phase"] - 2.0 * w * lag).max() <= 1e-5


def test_bulk_correction_removes_an_offset_added_to_one_ascan():
    X = dc.field(2, 10, 40, 42).astype(np.complex128)
    Y = X.copy()
    Y[:, 4] *= np.exp(1j * 1.1)          # one A-scan of every frame turned by a constant
    a = dm.model(X, dm.ASCANS, 1, (1, 1), bulk=True, truth=True)
    b = dm.model(Y, dm.ASCANS, 1, (1, 1), bulk=True, truth=True)
    scale = np.abs(a["corr"]).max()
    assert np.abs(a["corr"] - b["corr"]).max() <= 1e-12 * scale
    plain = dm.model(Y, dm.ASCANS, 1, (1, 1), truth=True)
    assert np.abs(plain["corr"] - dm.model(X, dm.ASCANS, 1, (1, 1), truth=True)["corr"]).max() > 0.1 * scale   # without it the offset is there
    # the corrected rows' bulk sums are real and positive: the correction takes the rows' common phase out
    Bc = b["corr"].sum(-1)
    assert np.abs(np.angle(Bc)).max() <= 1e-9
    # a row of zeros: B = 0, T' = T = 0
    Y[0, 7] = 0
    z = dm.model(Y, dm.ASCANS, 1, (1, 1), bulk=True, truth=True)
    assert np.all(z["corr"][0, 6:8] == 0) and np.all(z["phase"][0, 6:8] == 0) and np.isfinite(z["corr"]).all()


def test_edge_counts():
    assert dm.count(5, 6, 1, 1).tolist() == np.ones((5, 6), int).tolist()
    c = dm.count(5, 6, 3, 4)    # rows [r - 1, r + 1], depths [b - 1, b + 2]
    assert c[:, 0].tolist() == [2 * 3, 3 * 3, 3 * 3, 3 * 3, 2 * 3]
    assert c[2].tolist() == [3 * 3, 3 * 4, 3 * 4, 3 * 4, 3 * 3, 3 * 2]
    c = dm.count(3, 2, 32, 32)  # beyond the image both ways: all of it, everywhere
    assert np.all(c == 6)
    c = dm.count(40, 1, 4, 8)   # rows [r - 1, r + 2]
    assert c[:, 0].tolist() == [3, 4] + [4] * 35 + [4, 3, 2]
    ones = np.ones((2, 7, 9))
    np.testing.assert_array_equal(dm.box(ones, 4, 5)[0], dm.count(7, 9, 4, 5))
