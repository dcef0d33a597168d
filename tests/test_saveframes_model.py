"""CPU tests of tests/saveframes_model.py, the specification of include/fdoct_saveframes.h: the picture against the oracle's
display, the fold against a literal restatement of BscanFFT.cpp:1197-1240, and the construction of the shared test inputs --
no pixel of any of them lies near enough to a rounding tie for a device's last double bits to decide a byte."""
import numpy as np
import pytest

import oracle_lib as orc
import saveframes_model as m

SHAPES = m.PICTURE_SHAPES + tuple(sh for sh, _ in m.EXTRA_PICTURE_SETS if sh not in m.PICTURE_SHAPES) + (m.BIG_SHAPE,)


def _inputs(shape):
    """Every image the GPU tests make pictures of at this shape, as (name, (H, D) image)."""
    if shape == m.BIG_SHAPE:
        return [("big", m.frames_hd(shape, 1, first=1)[0])]
    out = [("3 frames, image %d" % k, f) for k, f in enumerate(m.frames_hd(shape, 3))]
    out += [("1 frame, kind %d" % k, m.frames_hd(shape, 1, first=k)[0]) for k in range(3)]
    for sh, n in m.EXTRA_PICTURE_SETS:
        if sh == shape:
            out += [("%d frames, image %d" % (n, k), f) for k, f in enumerate(m.frames_hd(sh, n))]
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_picture_equals_the_oracle_display_of_the_transposed_db(shape):
    for name, f in _inputs(shape):
        d = 20.0 * np.log(f.T.astype(np.float64) + 0.000001) / 2.303
        want = orc.display_u8(d, thr=-1e300, clampupper=False)
        got = m.image(f, m.ROWMAJOR)
        assert got.shape == (shape[1], shape[0]) and np.array_equal(got, want), name
        assert np.array_equal(m.image(np.ascontiguousarray(f.T), m.TRANSPOSED), want), name + ", D x H input"


def test_degenerate_pictures_and_the_clamp():
    assert not m.image(np.full((5, 9), 3.25, np.float32), m.ROWMAJOR).any()
    assert not m.image(np.zeros((9, 5), np.float32), m.TRANSPOSED).any()
    neg = np.array([[-1.0, 0.0, 1.0]], np.float32)          # the negative input reads as a zero does
    assert np.array_equal(m.image(neg, m.TRANSPOSED), m.image(np.array([[0.0, 0.0, 1.0]], np.float32), m.TRANSPOSED))
    two = m.image(np.array([[0.0, 7.0]], np.float32), m.TRANSPOSED)
    assert two.tolist() == [[0, 255]]


def _literal_fold(frames_hd, averages, eps, dc_mask):
    """main:1193-1240 image by image on (H, D) frames: bscantransposed accumulates H x D, bscan is its transpose."""
    H, D = frames_hd.shape[1:]
    out_b, out_db = [], []
    bscantransposed = np.zeros((H, D), np.float64)
    indextemp = 0
    for magI in frames_hd:
        bscantemp = magI.astype(np.float64)                  # 1195-1196
        bscantransposed += bscantemp                         # 1197
        indextemp += 1
        if indextemp >= averages:
            indextemp = 0
            bscan = bscantransposed.T.copy()                 # 1220
            bscan = bscan / averages                         # 1221
            bscan += eps                                     # 1222
            bscanlog = np.log(bscan)                         # 1235
            bscandb = 20.0 * bscanlog / 2.303                # 1237
            if dc_mask and D > 4:
                bscandb[1] = bscandb[4]                      # 1239
                bscandb[0] = bscandb[4]                      # 1240
            out_b.append(bscan.astype(np.float32)), out_db.append(bscandb.astype(np.float32))
            bscantransposed = np.zeros((H, D), np.float64)   # 1482
    return np.array(out_b), np.array(out_db)


@pytest.mark.parametrize("averages,n", [(1, 5), (3, 15), (5, 5), (5, 15)])
@pytest.mark.parametrize("D", [4, 5, 37])
def test_fold_equals_the_literal_restatement(D, averages, n):
    H = 6
    f = m.fold_frames(n, H, D)
    for dc in (0, 1):
        want_b, want_db = _literal_fold(f, averages, m.EPS_MAIN, dc)
        outs = {}
        for il in (m.ROWMAJOR, m.TRANSPOSED):
            for ol in (m.ROWMAJOR, m.TRANSPOSED):
                b, db = m.fold(m.in_layout_of(f, il), averages, m.EPS_MAIN, dc, il, ol)
                if ol == m.ROWMAJOR:
                    b, db = np.transpose(b, (0, 2, 1)), np.transpose(db, (0, 2, 1))
                outs[il, ol] = (b, db)
                assert b.shape == (n // averages, D, H)
                assert np.array_equal(b.view(np.uint32), want_b.view(np.uint32)), (il, ol, dc)
                assert np.array_equal(db.view(np.uint32), want_db.view(np.uint32)), (il, ol, dc)
        if D > 4 and dc:
            db = outs[m.ROWMAJOR, m.TRANSPOSED][1]
            assert np.array_equal(db[:, 0], db[:, 4]) and np.array_equal(db[:, 1], db[:, 4])


@pytest.mark.parametrize("shape", SHAPES)
def test_no_shared_input_has_a_pixel_inside_the_tie_band(shape):
    """The GPU test demands equal bytes with no pixel left out; that is fair only if no unrounded model value lies within
    tie_band of a half-integer.  Lognormal magnitudes spread d over ~150 dB, so the band is ~5e-13 of a grey level and the nearest
    pixel of a million lies ~1e-7 away."""
    worst = np.inf
    for name, f in _inputs(shape):
        dist, band = m.tie_distance(f, m.ROWMAJOR)
        assert dist > band, "%s %s: a pixel %.3g from a tie, band %.3g" % (shape, name, dist, band)
        dist_t, band_t = m.tie_distance(np.ascontiguousarray(f.T), m.TRANSPOSED)
        assert (dist_t, band_t) == (dist, band)
        if band:
            worst = min(worst, dist / band)
            assert band < 1e-11
    print("shape %s: the nearest pixel is %.3g bands from a tie" % (shape, worst))


def test_the_shared_inputs_put_their_extrema_where_they_say():
    for shape in m.PICTURE_SHAPES[1:] + (m.BIG_SHAPE,):
        H, D = shape
        f0, f1 = m.frames_hd(shape, 1, first=0)[0], m.frames_hd(shape, 1, first=1)[0]
        assert f0.argmin() == 0 and f0.argmax() == H * D - 1 and (f0 == f0.min()).sum() == 1
        h1, d1 = np.unravel_index(f1.argmin(), f1.shape)
        assert (f1 == 0).sum() == 1 and f1.argmax() == H * D - 1
        assert (h1 >= m.TILE * ((H - 1) // m.TILE) and d1 >= m.TILE * ((D - 1) // m.TILE)) or (h1, d1) == (0, 0)
    f2 = m.frames_hd((67, 129), 1, first=2)[0]
    assert 0.02 < (f2 == 0).mean() < 0.08
    big = m.frames_hd(m.BIG_SHAPE, 1, first=1)[0]
    assert big.size > 256 * 4096 and big.argmin() >= 256 * 4096      # the extrema sit beyond what one capped pass reaches
