"""tests/manualavg_model.py, the specification of manual averaging (BscanFFT.cpp:1399-1444), against cases worked by hand."""
import numpy as np
import pytest

import manualavg_model as m


def _images(n=7, shape=(3, 5), seed=1):
    return np.random.default_rng(seed).uniform(1e-5, 50.0, (n,) + shape).astype(np.float32)


def _mean(*imgs):
    s = np.zeros(imgs[0].shape, np.float64)
    for b in imgs:
        s += b.astype(np.float64)
    return s / float(len(imgs))


def _expect(groups):
    means = [_mean(*g) for g in groups]
    return (np.array([q.astype(np.float32) for q in means]), np.array([(20.0 * np.log(q) / 2.303).astype(np.float32) for q in means]))


def test_reference_mode_drops_the_image_that_arrives_when_m_are_in():
    b = _images()
    avg = m.ManualAvg(2, 15)
    mean, db = avg.add(b)
    want_mean, want_db = _expect([(b[0], b[1]), (b[3], b[4])])   # emitted on the arrival of b2 and of b5, which enter no sum
    assert mean.shape == db.shape == (2, 3, 5) and mean.dtype == db.dtype == np.float32
    np.testing.assert_array_equal(mean, want_mean)
    np.testing.assert_array_equal(db, want_db)
    assert avg.accumulated == 1
    np.testing.assert_array_equal(avg.acc, b[6].astype(np.float64).ravel())   # b6 alone is left in the accumulator
    assert m.plan(2, m.REFERENCE, 0, 7) == (2, 1)


def test_keep_all_mode_emits_with_the_mth_image():
    b = _images()
    avg = m.ManualAvg(2, 15, m.KEEP_ALL)
    mean, db = avg.add(b)
    want_mean, want_db = _expect([(b[0], b[1]), (b[2], b[3]), (b[4], b[5])])
    np.testing.assert_array_equal(mean, want_mean)
    np.testing.assert_array_equal(db, want_db)
    assert avg.accumulated == 1
    np.testing.assert_array_equal(avg.acc, b[6].astype(np.float64).ravel())
    assert m.plan(2, m.KEEP_ALL, 0, 7) == (3, 1)


def test_m_1_reference_emits_every_second_image_unchanged():
    b = _images()
    avg = m.ManualAvg(1, 15)
    mean, _ = avg.add(b)
    np.testing.assert_array_equal(mean, b[[0, 2, 4]])            # b1, b3, b5 are dropped
    assert avg.accumulated == 1
    keep = m.ManualAvg(1, 15, m.KEEP_ALL)
    np.testing.assert_array_equal(keep.add(b)[0], b)
    assert keep.accumulated == 0


@pytest.mark.parametrize("mode", [m.REFERENCE, m.KEEP_ALL])
def test_every_split_into_two_calls_equals_one_call(mode):
    b = _images()
    one = m.ManualAvg(2, 15, mode)
    mean, db = one.add(b)
    for k in range(8):
        two = m.ManualAvg(2, 15, mode)
        first, second = two.add(b[:k]), two.add(b[k:])
        np.testing.assert_array_equal(np.concatenate([first[0], second[0]]), mean)
        np.testing.assert_array_equal(np.concatenate([first[1], second[1]]), db)
        assert two.accumulated == one.accumulated
        assert two.acc.tobytes() == one.acc.tobytes()
        e1, a1 = m.plan(2, mode, 0, k)
        e2, a2 = m.plan(2, mode, a1, 7 - k)
        assert (e1, e1 + e2, a2) == (first[0].shape[0], mean.shape[0], one.accumulated)


def test_a_mean_of_zero_is_minus_infinity_and_bad_arguments_raise():
    avg = m.ManualAvg(1, 4, m.KEEP_ALL)
    mean, db = avg.add(np.array([[0.0, 1.0, 2.303, 0.0]], np.float32))
    assert mean[0].tolist() == [0.0, 1.0, np.float32(2.303), 0.0]
    assert db[0, 0] == -np.inf and db[0, 3] == -np.inf and db[0, 1] == 0.0
    for bad in [(0, 0, 0, 1), (2, 2, 0, 1), (2, 0, 3, 1), (2, 0, -1, 1), (2, 0, 0, -1)]:
        with pytest.raises(ValueError):
            m.plan(*bad)
    assert m.plan(3, m.REFERENCE, 3, 1) == (1, 0) and m.plan(3, m.REFERENCE, 3, 0) == (0, 3)
