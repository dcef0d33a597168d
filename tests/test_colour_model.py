"""CPU tests of the colour front end's specification (tests/colour_model.py) against the oracle's restatements and against
exact arithmetic."""
import numpy as np
import pytest

import colour_model
import oracle_lib


def _frames(seed, n=2, h=60, w=120):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("mediann", colour_model.MEDIANS)
@pytest.mark.parametrize("bins", [(1, 1), (2, 2), (4, 4), (3, 1), (1, 2)])
def test_select_is_the_oracle_front_end_on_that_channel(c, mediann, bins):
    f = _frames(7 + c)
    got = colour_model.extract(f, c, mediann, *bins)
    assert got.dtype == np.uint8 and got.shape == (2, 60 // bins[1], 120 // bins[0])
    for i in range(f.shape[0]):
        m = np.ascontiguousarray(f[i, :, :, c])
        if mediann:
            m = oracle_lib.median_blur(m, mediann)
        assert np.array_equal(got[i], oracle_lib.resize_area(m, *bins))


def test_select_without_median_or_binning_is_the_channel():
    f = _frames(3)
    for c in range(3):
        assert np.array_equal(colour_model.extract(f, c), f[..., c])


def test_sum_without_binning_is_the_reference_line_in_float64_bit_for_bit():
    f = np.concatenate([_frames(11), np.zeros((1, 60, 120, 3), np.uint8), np.full((1, 60, 120, 3), 255, np.uint8)])
    b, g, r = (f[..., k].astype(np.float64) for k in range(3))
    want = (b + g + r) * 0.00130718954
    got = colour_model.extract(f, 3)
    assert got.dtype == np.float64 and np.array_equal(colour_model.bits(got), colour_model.bits(want))
    assert colour_model.SUM_SCALE == 0.00130718954 and colour_model.SUM_SCALE != 1.0 / 765.0
    assert not got[-2].any() and np.all(got[-1] == 765.0 * 0.00130718954) and got[-1].max() < 1.0  # 765 * the literal = 1 - 1.9e-9


def test_sum_rejects_a_median():
    with pytest.raises(AssertionError):
        colour_model.extract(_frames(1), 3, mediann=3)


# Largest distance of the reference-mode binning from exact arithmetic, in ulps of the exact result, measured on the frames of
# seeds 100 .. 103 (2 x 60 x 120 each): the figure and twice it, the bound asserted.  For power-of-two areas 1.f / area is
# exact and what remains is the rounding of the area's additions; otherwise the float reciprocal's own error dominates,
# |float32(1 / area) * area - 1| = 2.98e-8 (area 3) and 5.22e-8 (area 15), i.e. 2.7e8 and 4.7e8 ulps.
MEASURED_ULPS = {(2, 2): 2.0, (4, 4): 3.0, (3, 1): 268318492.0, (5, 3): 469639233.0}


@pytest.mark.parametrize("bins", sorted(MEASURED_ULPS))
def test_sum_binning_reference_mode_stays_within_twice_the_measured_distance_from_truth(bins):
    """Measured worst cases (seeds 100-103): 2 x 2: 2 ulps; 4 x 4: 3 ulps; 3 x 1: 2.68318492e8 ulps; 5 x 3: 4.69639233e8 ulps
    (the last two are the error of (double)(1.f / area) itself)."""
    worst = 0.0
    for seed in range(100, 104):
        f = _frames(seed)
        ref = colour_model.extract(f, 3, 0, *bins)
        truth = colour_model.extract(f, 3, 0, *bins, mode="truth")
        worst = max(worst, float(colour_model.ulps(ref, truth).max()))
    print("bins %s: worst %.9g ulps" % (bins, worst))
    assert worst <= 2.0 * MEASURED_ULPS[bins]
    # all-zero and all-255 frames: 0 exactly, and the same bound
    z = np.zeros((1, 60, 120, 3), np.uint8)
    assert not colour_model.extract(z, 3, 0, *bins).any()
    s = np.full((1, 60, 120, 3), 255, np.uint8)
    assert colour_model.ulps(colour_model.extract(s, 3, 0, *bins), colour_model.extract(s, 3, 0, *bins, mode="truth")).max() <= 2.0 * MEASURED_ULPS[bins]
