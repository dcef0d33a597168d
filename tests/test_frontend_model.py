"""CPU tests of tests/frontend_model.py, the numpy / scipy statement of the camera front end and the display post-chain, against
the oracle's own restatements (oracle_lib: orc_median_blur_u16, orc_resize_area_u16, orc_display_u8, orc_apply_lut,
orc_lockin_db) on the small frames, the constructed rounding ties and the bin factors that tests/test_gpu_frontend_edges.py
uses.  Bit-for-bit agreement here is what licenses that file to take the model alone as its reference at shapes where the
oracle's per-pixel qsort would take minutes.

Had the two disagreed, OpenCV's documented behaviour would decide: cv::medianBlur replicates the border (BORDER_REPLICATE) and
returns the middle of the sorted window; cv::resize(INTER_AREA) at an integer factor is the block mean, rounded to the nearest
sample by saturate_cast (round half to even) except in the vectorised 2 x 2 path of 8- and 16-bit images, which computes
(s + 2) >> 2.  They agree everywhere below, so nothing had to be decided."""
import numpy as np
import pytest

import frontend_model as fm
import oracle_lib as orc

DTYPES = (np.uint8, np.uint16)
GPU_BINS = ((3, 1), (1, 2), (2, 2))  # the factors of the second-pass cases of tests/test_gpu_frontend_edges.py


def _orc_median(frames, n):
    return np.stack([orc.median_blur(f, n) for f in frames]).astype(frames.dtype)


def _orc_bin(frames, binx, biny):
    return np.stack([orc.resize_area(f, binx, biny) for f in frames]).astype(frames.dtype)


def _sorted_window_median(frame, n):
    """The definition, without scipy or the oracle: edge-pad, sort every window, take the middle."""
    r = n // 2
    p = np.pad(frame, r, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(p, (n, n)).reshape(frame.shape + (n * n,))
    return np.sort(win, axis=-1)[..., n * n // 2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (3, 5, 7))
@pytest.mark.parametrize("shape", fm.SMALL_SHAPES + ((21, 37),))
def test_median_model_is_the_oracle_and_the_sorted_window(dtype, n, shape):
    frames = fm.small_frames(dtype, *shape)
    got = fm.median(frames, n)
    assert got.dtype == dtype and got.shape == frames.shape
    np.testing.assert_array_equal(got, _orc_median(frames, n))
    np.testing.assert_array_equal(got, np.stack([_sorted_window_median(f, n) for f in frames]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", fm.SMALL_BINS)
def test_bin_model_is_the_oracle_on_frames_of_a_few_blocks(dtype, bins):
    frames = fm.small_frames(dtype, *fm.SMALL_BIN_SHAPE)
    got = fm.bin_area(frames, *bins)
    assert got.dtype == dtype and got.shape == (3, fm.SMALL_BIN_SHAPE[0] // bins[1], fm.SMALL_BIN_SHAPE[1] // bins[0])
    np.testing.assert_array_equal(got, _orc_bin(frames, *bins))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", fm.TIE_BINS + GPU_BINS + fm.SMALL_BINS)
def test_bin_model_is_the_oracle_on_random_frames(dtype, bins):
    rng = np.random.default_rng(17 * bins[0] + bins[1])
    frames = rng.integers(0, np.iinfo(dtype).max + 1, (2, 12 * bins[1], 14 * bins[0])).astype(dtype)
    np.testing.assert_array_equal(fm.bin_area(frames, *bins), _orc_bin(frames, *bins))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", fm.TIE_BINS)
def test_constructed_ties_round_half_to_even(dtype, bins):
    """Every block of an even area sums to area * q + area / 2: the mean is q + 1/2 and goes to the even neighbour, q + (q & 1).
    float32(1 / area) is exact for areas 2, 4 and 8; for 6 and 12 it is 1/6 resp. 1/12 times (1 + 2^-25), which moves q + 1/2 by
    less than half a float32 spacing for every 16-bit q, so the product rounds back onto the tie.  Area 3 has no ties: the blocks
    sum to 3 q + 1 and 3 q + 2, the nearest thirds, and go to q and q + 1."""
    frame, qs = fm.tie_frame(dtype, *bins)
    area = bins[0] * bins[1]
    got = fm.bin_area(frame, *bins)
    np.testing.assert_array_equal(got, _orc_bin(frame[None], *bins)[0])
    if area % 2 == 0:
        assert fm.ties(frame, *bins).mean() >= 0.25
        assert fm.ties(frame, *bins).all()
        np.testing.assert_array_equal(got, qs + (qs & 1))
    else:
        want = qs.copy()
        want[:, 1::2] += 1
        np.testing.assert_array_equal(got, want)
    assert (qs % 2 == 0).any() and (qs % 2 == 1).any()
    assert qs.min() == 0 and qs.max() == np.iinfo(dtype).max - 1 and ((qs > np.iinfo(dtype).max // 2 - 4) & (qs < np.iinfo(dtype).max // 2 + 4)).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wblocks", sorted(fm.TIE_2X2_WBLOCKS.values()))
def test_constructed_2x2_ties_round_up(dtype, wblocks):
    """2 x 2 is (s + 2) >> 2: s = 4 q + 2 goes to q + 1 whatever q's parity, up to the top of the sample range."""
    frame, qs = fm.tie_frame(dtype, 2, 2, wblocks)
    assert fm.ties(frame, 2, 2).all()
    got = fm.bin_area(frame, 2, 2)
    np.testing.assert_array_equal(got, qs + 1)
    np.testing.assert_array_equal(got, _orc_bin(frame[None], 2, 2)[0])
    assert got.max() == np.iinfo(dtype).max


def test_bin_model_refuses_16_bit_areas_beyond_exact_float32_sums():
    fm.bin_area(np.zeros((16, 16), np.uint16), 16, 16)
    fm.bin_area(np.zeros((32, 16), np.uint8), 16, 32)
    with pytest.raises(AssertionError):
        fm.bin_area(np.zeros((32, 16), np.uint16), 16, 32)


def _db(rng, shape, lo=-70.0, hi=40.0):
    return rng.uniform(lo, hi, shape).astype(np.float32)


@pytest.mark.parametrize("shape", ((1, 1), (1, 2), (1, 3), (1, 5), (1, 7), (3, 85), (6, 6), (64, 40)))
def test_display_and_lut_model_is_the_oracle(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    table = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    db = _db(rng, shape)
    for thr in (-30.0, -10.0, -1e9, 1e3):
        for clamp in ((False, True) if min(shape) > 5 else (False,)):
            got = fm.display(db, thr, clamp)
            np.testing.assert_array_equal(got, orc.display_u8(db.astype(np.float64), thr, clamp))
            np.testing.assert_array_equal(fm.lut(got, table), orc.apply_lut(got, table))
    with_inf = db.copy()
    with_inf.flat[::3] = -np.inf
    np.testing.assert_array_equal(fm.display(with_inf, -30.0), orc.display_u8(with_inf.astype(np.float64), -30.0, False))


def test_display_model_degenerate_ranges():
    rng = np.random.default_rng(5)
    db = _db(rng, (6, 6), -100.0, -40.0)
    assert not fm.display(db, -30.0).any()                       # threshold above every pixel: range 0, scale 0
    want = np.zeros((6, 6), np.uint8)
    want[5, 5] = 255
    np.testing.assert_array_equal(fm.display(db, -30.0, True), want)
    assert not fm.display(np.full((1, 1), 7.0, np.float32)).any()


def test_lockin_model_is_the_oracle_and_floors_exactly():
    rng = np.random.default_rng(6)
    b = np.abs(rng.standard_normal((3, 33, 7))).astype(np.float32)
    j = np.abs(rng.standard_normal((33, 7))).astype(np.float32)
    b[1, 4] = j[4]
    got = fm.lockin(b, j)
    want = np.stack([orc.lockin_db(x.astype(np.float64), j.astype(np.float64)) for x in b])
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-5)   # the project's figure (test_display_chain_bit_exact_and_lockin)
    assert got.dtype == np.float32 and (b <= j).any() and np.all(got[b <= j] == fm.LOCKIN_FLOOR)
