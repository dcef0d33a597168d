"""The 1024-point fast path (W = N = 2048) on the smallest batches where its lane-0 arithmetic and its epilogue can go wrong.

Lane 0 of a wave owns depth bins 0, 64, 128, ... and the self-paired bin NC/2 = 512, whose magnitude does not go through the
untangle's general formula but through |2 Z[NC/2]| (and shares the square root of lane 0's slot); the epsilon add works on
pairs of slots.  Batches: 3 rows in one frame (fewer rows than waves, and lane 0's bins are a visible share of the image), and
two frames of 1030 rows = 2060 rows (more than one pass of the 2048 row slots, ragged last pass).  Depths: all 1024 bins, the
half-depth 512 (bin NC/2 is cropped away) and a ragged 1000.  u16 and u8, both division settings, DC mask on and off,
row-major and D x H, fused and staged (staged mode takes u16 only).

Every case: helpers.check_mag / check_db against the oracle; D x H = row-major and staged = fused bit for bit; and lane 0's
bins of the dB image against 20 ln(x) / 2.303 of the SAME launch's linear image, within the oracle's dB tolerance."""
import functools

import numpy as np
import pytest

import helpers
from fdoct_amd import LAYOUT_TRANSPOSED, Config, Reconstructor, synth

pytestmark = pytest.mark.gpu

W = N = 2048
NC, T = N // 2, 64
BATCHES = {"3 rows": (3, 1), "2060 rows": (1030, 2)}   # name -> (rows per frame, frames)
DEPTHS = (1024, 512, 1000)


@functools.lru_cache(maxsize=None)
def _inputs(batch, dt):
    H, nframes = BATCHES[batch]
    frames, yb = synth.make_frames(7, nframes, W, H, dtype=dt), synth.make_background(W, dtype=dt)
    frames.setflags(write=False)
    yb.setflags(write=False)
    return frames, yb


@functools.lru_cache(maxsize=None)
def _oracle(batch, dt, D):
    """(linear (G, H, D), dB (G, H, D) with the DC mask, dB without it) -- computed once per shape, read-only."""
    frames, yb = _inputs(batch, dt)
    mag, _, db = helpers.oracle_reference(Config(width=W, height=BATCHES[batch][0], numfftpoints=N, numdisplaypoints=D), frames, yb)
    db = np.ascontiguousarray(np.transpose(db, (0, 2, 1)))
    # without the mask, depth bins 0 and 1 are what main:1235-1237 makes of the oracle's own linear bins
    db_nomask = db.copy()
    db_nomask[..., :2] = 20.0 * np.log(mag[..., :2].astype(np.float64)) / 2.303
    for a in (mag, db, db_nomask):
        a.setflags(write=False)
    return mag, db, db_nomask


def _lane0_bins(D):
    """Depth bins of lane 0 below D: l + T*m for l = 0, their mirror images NC - T*m, and the self-paired NC/2 among them."""
    return np.arange(0, min(D, NC), T)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("dt", [np.uint16, np.uint8], ids=["u16", "u8"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_lane0_bins_epilogue_and_layouts(batch, dt, D):
    H, nframes = BATCHES[batch]
    frames, yb = _inputs(batch, dt)
    mag_o, db_o, db_o_nomask = _oracle(batch, dt, D)
    bins = _lane0_bins(D)
    assert (NC // 2 in bins) == (D > NC // 2)
    for dc_mask in (1, 0):
        for precise in (True, False):
            what = "%s %s D=%d dc_mask=%d %s division" % (batch, np.dtype(dt).name, D, dc_mask, "two-word" if precise else "one-word")
            r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, dc_mask=dc_mask))
            r.set_background(yb)
            r.set_precise_division(precise)
            b, d = r.process(frames)
            bt, dtr = r.process(frames, layout=LAYOUT_TRANSPOSED)
            if dt == np.uint16:
                r.set_staged(True)
                bs, ds = r.process(frames)
                t = r.timing()
            r.close()
            assert b.shape == (nframes, H, D) and d.shape == (nframes, H, D)
            # D x H = row-major, staged = fused: bit for bit
            np.testing.assert_array_equal(bt, np.transpose(b, (0, 2, 1)), what + ": D x H linear")
            np.testing.assert_array_equal(dtr, np.transpose(d, (0, 2, 1)), what + ": D x H dB")
            if dt == np.uint16:
                assert t["resample_stage_ms"] > 0 and t["fft_stage_ms"] > 0
                np.testing.assert_array_equal(bs, b, what + ": staged linear")
                np.testing.assert_array_equal(ds, d, what + ": staged dB")
            # the oracle, every bin
            db_ref = db_o if dc_mask else db_o_nomask
            w_mag = helpers.check_mag(b, mag_o, what)
            w_db = helpers.check_db(d, db_ref, mag_o, what)
            # lane 0's bins on their own: linear against the oracle, dB against the scalar formula on this launch's linear image
            w_l0 = float(helpers.mag_ratio(b, mag_o)[..., bins].max())
            db_scalar = 20.0 * np.log(b.astype(np.float64)) / 2.303
            if dc_mask:
                db_scalar[..., 0] = db_scalar[..., 1] = db_scalar[..., 4]     # depth bins 0 and 1 carry bin 4 (main:1237-1238)
            w_l0_db = float(helpers.db_ratio(d, db_scalar, mag_o)[..., bins].max())
            print("%s: err/tol linear %.3f dB %.3f; lane 0's bins linear %.3f, dB vs the scalar formula %.3f" % (what, w_mag, w_db, w_l0, w_l0_db))
            assert w_l0 <= 1.0, "%s: lane 0's bins, worst linear error/tolerance %.3g" % (what, w_l0)
            assert w_l0_db <= 1.0, "%s: lane 0's bins, dB against 20 ln(x)/2.303 of the same launch: error/tolerance %.3g" % (what, w_l0_db)
            if dc_mask and D > 4:
                np.testing.assert_array_equal(d[..., 0], d[..., 4], what + ": depth bin 0 is bin 4")
                np.testing.assert_array_equal(d[..., 1], d[..., 4], what + ": depth bin 1 is bin 4")

