"""CPU tests of tests/bscanbin_model.py, the specification of spinjnt's output binning (include/fdoct_bscanbin.h): the cubic's
taps, the constant image, the loop-literal model against an independent dense-matrix formulation, the distance between its
"reference" precision and the double one, and -- for a maintainer who has OpenCV -- tools/make_opencv_golden.cpp's vectors."""
import glob
import os

import numpy as np
import pytest

import bscanbin_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _peaked(D, H, seed):
    """Reflector peaks on a floor, like a linear B-scan: the cubic undershoots beside them."""
    rng = np.random.default_rng(seed)
    pic = rng.uniform(0.5, 1.5, (D, H))
    for _ in range(max(3, D * H // 400)):
        pic[rng.integers(D), rng.integers(H)] += rng.uniform(200, 3000)
    return pic.astype(np.float32)


def test_taps_sum_to_one_and_u1_is_the_identity():
    for mode in ("truth", "reference"):
        for u in range(1, m.MAX_UP + 1):
            c, off = m.taps(u, mode)
            assert c.shape == (u, 4) and np.abs(c.sum(axis=1) - 1).max() <= (1e-15 if mode == "truth" else 2e-7)
            assert set(off) <= {-2, -1}
        c, off = m.taps(1, mode)
        assert c.tolist() == [[0.0, 1.0, 0.0, 0.0]] and off.tolist() == [-1]
    pic = _peaked(12, 20, 1)
    lin, _ = m.bscan_bin(pic, 1, 1)
    np.testing.assert_array_equal(lin, pic.astype(np.float64))


def test_a_constant_image_comes_out_as_constant_times_multiplyfactor():
    for binx, biny, upx, upy, mf in [(2, 2, 2, 2, 4), (3, 1, 3, 1, 3), (1, 4, 1, 4, 4), (2, 1, 4, 1, 8), (5, 3, 5, 3, 15.0), (16, 16, 16, 16, 256)]:
        pic = np.full((biny * 6, binx * 7), 3.25, np.float32)
        for mode in ("truth", "reference"):
            lin, _ = m.bscan_bin(pic, binx, biny, upx, upy, mf, mode=mode)
            assert lin.shape == m.out_size(biny * 6, binx * 7, binx, biny, upx, upy)
            assert np.abs(lin - 3.25 * mf).max() <= 3.25 * mf * (1e-14 if mode == "truth" else 5e-7)


CASES = [  # depths, ascans, binx, biny, upx, upy
    (24, 36, 2, 2, 2, 2), (10, 30, 3, 1, 3, 1), (32, 9, 1, 4, 1, 4), (12, 20, 2, 1, 4, 1), (16, 16, 4, 4, 4, 4), (15, 25, 5, 3, 5, 3),
    (32, 48, 16, 16, 16, 16), (7, 11, 1, 1, 1, 1), (2, 12, 4, 2, 8, 4),  # binned sizes 1 x 3
    (6, 4, 2, 3, 2, 3), (9, 2, 2, 3, 2, 3),                             # 2 x 2, 3 x 1 cells
    (8, 12, 4, 2, 1, 1), (20, 12, 2, 2, 64, 3)]


@pytest.mark.parametrize("case", CASES)
def test_loop_literal_model_equals_the_dense_matrix_formulation(case):
    D, H, binx, biny, upx, upy = case
    pic = _peaked(D, H, D * 100 + H)
    mf = binx * biny * 1.5
    lin, _ = m.bscan_bin(pic, binx, biny, upx, upy, mf)
    want = m.dense(pic, binx, biny, upx, upy, mf)
    assert lin.shape == want.shape == m.out_size(D, H, binx, biny, upx, upy)
    assert np.abs(lin - want).max() <= 1e-12 * np.abs(want).max()
    j = _peaked(D, H, 5)
    lin_j, db_j = m.bscan_bin(pic, binx, biny, upx, upy, mf, jscan=j)
    want_j = m.dense(np.maximum(pic.astype(np.float64) - j, 0) + 0.001, binx, biny, upx, upy, mf)
    assert np.abs(lin_j - want_j).max() <= 1e-12 * np.abs(want_j).max() and np.isfinite(db_j).all()


def test_reference_precision_stays_within_the_tolerance_of_truth():
    worst = {}
    for binx, biny, upx, upy in [(1, 1, 1, 1), (2, 2, 2, 2), (3, 1, 3, 1), (1, 4, 1, 4), (2, 1, 4, 1), (4, 4, 4, 4), (5, 3, 5, 3), (16, 16, 16, 16)]:
        pic = _peaked(240, 240, 7)
        truth, _ = m.bscan_bin(pic, binx, biny, upx, upy)
        ref, _ = m.bscan_bin(pic, binx, biny, upx, upy, mode="reference")
        worst[(binx, biny, upx, upy)] = float((np.abs(ref - truth) / m.tolerance(truth)).max())
        print("reference vs truth, bin %d x %d up %d x %d: %.3f x tol; truth <= 0 on %.2f %% of the elements" % (
            binx, biny, upx, upy, worst[(binx, biny, upx, upy)], 100 * (truth <= 0).mean()))
    assert max(worst.values()) < 1.0
    assert worst[(2, 2, 2, 2)] < 0.01 and worst[(4, 4, 4, 4)] < 0.01   # powers of two: the float32 taps and 1 / area are exact


def test_undershoot_and_the_db_clamp():
    pic = _peaked(96, 128, 3)
    lin, db = m.bscan_bin(pic, 2, 2)
    assert (lin <= 0).mean() > 0.005 and np.isfinite(db).all()
    assert (db[2:][lin[2:] <= 0] == 20.0 * np.log(m.EPS_MAIN) / 2.303).all()
    np.testing.assert_array_equal(db[0], db[4])
    np.testing.assert_array_equal(db[1], db[4])
    _, db_nomask = m.bscan_bin(pic, 2, 2, dc_mask=False)
    assert not np.array_equal(db_nomask[0], db_nomask[4])
    _, db_j = m.bscan_bin(pic, 2, 2, jscan=np.zeros_like(pic))
    assert not np.array_equal(db_j[0], db_j[4])          # no mask behind the lock-in
    _, db4 = m.bscan_bin(pic[:8], 1, 2, upy=1)            # out_depths == 4: rows unmasked
    assert db4.shape[0] == 4 and np.array_equal(db4, m.bscan_bin(pic[:8], 1, 2, upy=1, dc_mask=False)[1])


def test_opencv_golden_vectors_if_present():
    """tools/make_opencv_golden.cpp writes tests/golden/opencv_bscanbin_<binx>x<biny>_bv<binvaluey>.bin from the two resize
    calls: int32 header (depths, ascans, binx, biny, upx, upy, out_depths, out_ascans), float64 multiplyfactor, the float32
    input and the float64 result.  OpenCV pins the reference mode to rounding; this project cannot produce them."""
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "opencv_bscanbin_*.bin")))
    if not files:
        pytest.skip("no tests/golden/opencv_bscanbin_*.bin (written by tools/make_opencv_golden.cpp where OpenCV is installed)")
    for f in files:
        raw = open(f, "rb").read()
        D, H, binx, biny, upx, upy, od, oa = np.frombuffer(raw, np.int32, 8)
        mf = float(np.frombuffer(raw, np.float64, 1, 32)[0])
        pic = np.frombuffer(raw, np.float32, D * H, 40).reshape(D, H)
        want = np.frombuffer(raw, np.float64, od * oa, 40 + 4 * D * H).reshape(od, oa)
        ref, _ = m.bscan_bin(pic, binx, biny, upx, upy, mf, mode="reference")
        assert (np.abs(ref - want) <= 1e-9 * np.abs(want).max()).all(), f
