"""GPU tests of the camera front end (fdoct_generic.hip: median_kernel, median3_fast_kernel, bin_kernel, bin2x2_kernel) and of the
display post-chain (fdoct_display.hip: display_minmax_kernel, display_map_kernel, lockin_db_kernel) where the launch code takes
another path than in tests/test_gpu_parity.py: inputs larger than one pass of a fixed grid, frames smaller than the median's
window, block sums that are exact rounding ties, misaligned device pointers, images beyond the cap of partial minima and
maxima, and images of fewer pixels than a wave has lanes.  The reference is tests/frontend_model.py (numpy and scipy), which
tests/test_frontend_model.py holds to the oracle bit for bit on the CPU; every comparison but the lock-in's is exact."""
import numpy as np
import pytest

import frontend_model as fm
import oracle_lib as orc
from fdoct_amd import Config, Reconstructor, capi

pytestmark = pytest.mark.gpu

# What one pass of each fixed launch covers.  The shapes below are worked out from these figures, so that a change of a grid
# moves the shapes with it: keep them equal to the launch code.
MEDIAN_PASS = 8192 * 256      # pixels: median_kernel, dim3 g(8192), b(256)                       fdoct_generic.hip:901
MEDIAN3_ROWS = 32768          # rows: median3_fast_kernel, the cap of gridDim.y                   fdoct_generic.hip:897
BIN_PASS = 4096 * 256         # outputs: bin_kernel, dim3(4096), dim3(256)                        fdoct_generic.hip:969, :972
BIN2X2_PASS = 8192 * 256      # 16-byte vectors: bin2x2_kernel, dim3(8192), dim3(256)             fdoct_generic.hip:962, :964
DISP_PART_PIXELS = 256 * 16   # pixels per part below the cap: DISP_BLOCK * 16, display_parts()   fdoct_display.hip:22, :179
DISP_MAX_PARTS = 256          # partial (min, max) pairs per B-scan                               fdoct_display.hip:23


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=8, numfftpoints=64, numdisplaypoints=32))  # (the geometry is irrelevant to these calls)
    yield r
    r.close()


def _random(dtype, shape, seed):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, shape, dtype=dtype)


# ---------------------------------------------------------------------------------------------- second pass of a fixed grid

def _median_h(w, nframes=2):
    return MEDIAN_PASS // (nframes * w) + (8 if w % 8 == 0 else 1)


@pytest.mark.parametrize("dtype,n,w", [(np.uint8, 5, 1024), (np.uint8, 7, 1024), (np.uint16, 5, 1024), (np.uint8, 3, 1028)])
def test_median_kernel_second_grid_pass(rec, dtype, n, w):
    """2 frames of 1032 x 1024 (1021 x 1028 for the 3 x 3 median, whose width keeps it off median3_fast_kernel): just over the
    2 097 152 pixels of one pass, so the last rows of the second frame, its lower border among them, come from the second one."""
    h = _median_h(w)
    raw = _random(dtype, (2, h, w), 40 + n)
    assert MEDIAN_PASS < raw.size < MEDIAN_PASS + MEDIAN_PASS // 64
    np.testing.assert_array_equal(rec.frontend(raw, n, 1, 1), fm.median(raw, n))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_median3_fast_kernel_beyond_the_row_cap(rec, dtype):
    """3 frames of 16 400 rows of 8 pixels: 49 200 rows against a grid of 32 768, with both frame borders inside the second pass."""
    h = MEDIAN3_ROWS // 2 + 16
    raw = _random(dtype, (3, h, 8), 50)
    assert MEDIAN3_ROWS < 3 * h and h < MEDIAN3_ROWS < 2 * h + h // 2
    raw[1, 0], raw[1, -1], raw[2, 0], raw[2, -1] = np.iinfo(dtype).max, 0, 0, np.iinfo(dtype).max
    np.testing.assert_array_equal(rec.frontend(raw, 3, 1, 1), fm.median(raw, 3))


@pytest.mark.parametrize("dtype,binx,biny,ow", [(np.uint8, 3, 1, 1026), (np.uint16, 1, 2, 1026), (np.uint8, 2, 2, 1030)])
def test_bin_kernel_second_grid_pass(rec, dtype, binx, biny, ow):
    """Raw 1024 x 3078 (3 x 1), 2048 x 1026 (1 x 2) and 2040 x 2060 (2 x 2, a row that is not whole 16-byte vectors: bin_kernel's
    own 2 x 2 branch): each just over the 1 048 576 outputs of one pass."""
    oh = -(-(BIN_PASS + 1) // ow) + 1
    raw = _random(dtype, (1, oh * biny, ow * binx), 60 + binx)
    assert (ow * binx * raw.itemsize) % 16 != 0 or (binx, biny) != (2, 2)
    assert BIN_PASS < oh * ow < BIN_PASS + BIN_PASS // 64
    np.testing.assert_array_equal(rec.frontend(raw, 0, binx, biny), fm.bin_area(raw, binx, biny))


def test_bin2x2_kernel_second_grid_pass(rec):
    """4 frames of 4128 x 4096, 8-bit: 2 113 536 vectors against 2 097 152 per pass (68 MB of raw frames)."""
    w = 4096
    h = 2 * (BIN2X2_PASS // (4 * (w // 16)) + 16)
    raw = _random(np.uint8, (4, h, w), 70)
    assert BIN2X2_PASS < 4 * (h // 2) * (w // 16) < BIN2X2_PASS + BIN2X2_PASS // 64
    np.testing.assert_array_equal(rec.frontend(raw, 0, 2, 2), fm.bin_area(raw, 2, 2))


def test_bin2x2_kernel_16_bit(rec):
    raw = _random(np.uint16, (2, 64, 1024), 71)
    np.testing.assert_array_equal(rec.frontend(raw, 0, 2, 2), fm.bin_area(raw, 2, 2))


# ---------------------------------------------------------------------------------------- frames smaller than the window

@pytest.mark.parametrize("dtype,n", [(np.uint8, 3), (np.uint8, 5), (np.uint8, 7), (np.uint16, 3), (np.uint16, 5)])
@pytest.mark.parametrize("shape", fm.SMALL_SHAPES)
def test_median_of_frames_smaller_than_the_window(rec, dtype, n, shape):
    """The replicated border clamps on both sides at once; three frames of different content, so that a row taken from the
    neighbouring frame shows."""
    raw = fm.small_frames(dtype, *shape)
    np.testing.assert_array_equal(rec.frontend(raw, n, 1, 1), fm.median(raw, n))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("bins", fm.SMALL_BINS)
def test_binning_of_frames_of_a_few_blocks(rec, dtype, bins):
    raw = fm.small_frames(dtype, *fm.SMALL_BIN_SHAPE)
    np.testing.assert_array_equal(rec.frontend(raw, 0, *bins), fm.bin_area(raw, *bins))


# ------------------------------------------------------------------------------------------------------- rounding ties

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("bins", fm.TIE_BINS)
def test_bin_kernel_rounds_ties_to_even(rec, dtype, bins):
    """Areas 2, 3, 4 (4 x 1 and 1 x 4), 6, 8 and 12, in both orientations: every block sum of the constructed frame is an exact tie
    (area 3, which has none: the nearest thirds), quotients even and odd at the bottom, the middle and the top of the sample
    range; then one seeded random frame of the same factor."""
    frame, qs = fm.tie_frame(dtype, *bins)
    got = rec.frontend(frame, 0, *bins)[0]
    np.testing.assert_array_equal(got, fm.bin_area(frame, *bins))
    if (bins[0] * bins[1]) % 2 == 0:
        assert fm.ties(frame, *bins).mean() >= 0.25   # (guards the construction, not the kernel)
        np.testing.assert_array_equal(got, qs + (qs & 1))
    raw = _random(dtype, (2, 12 * bins[1], 14 * bins[0]), 80 + bins[0])
    np.testing.assert_array_equal(rec.frontend(raw, 0, *bins), fm.bin_area(raw, *bins))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("kernel", sorted(fm.TIE_2X2_WBLOCKS))
def test_2x2_rounds_ties_up_on_both_kernels(rec, dtype, kernel):
    """(s + 2) >> 2: s = 4 q + 2 goes to q + 1, in bin2x2_kernel (rows of whole 16-byte vectors) and in bin_kernel's 2 x 2 branch."""
    wblocks = fm.TIE_2X2_WBLOCKS[kernel]
    frame, qs = fm.tie_frame(dtype, 2, 2, wblocks)
    assert ((2 * wblocks * frame.itemsize) % 16 == 0) == (kernel == "bin2x2_kernel")
    assert fm.ties(frame, 2, 2).mean() >= 0.25
    got = rec.frontend(frame, 0, 2, 2)[0]
    np.testing.assert_array_equal(got, fm.bin_area(frame, 2, 2))
    np.testing.assert_array_equal(got, qs + 1)
    raw = _random(dtype, (2, 24, 2 * wblocks), 90)
    np.testing.assert_array_equal(rec.frontend(raw, 0, 2, 2), fm.bin_area(raw, 2, 2))


# ------------------------------------------------------------------------------------------------------------- display

def _check_display(rec, db, thr, clamp, table, with_oracle=False):
    gray, bgr = rec.display(db, thr, clamp, colour=True)
    for b in range(db.shape[0]):
        want = fm.display(db[b], thr, clamp)
        np.testing.assert_array_equal(gray[b], want)
        np.testing.assert_array_equal(bgr[b], fm.lut(want, table))
        if with_oracle:
            np.testing.assert_array_equal(gray[b], orc.display_u8(db[b].astype(np.float64), thr, clamp))
    return gray, bgr


@pytest.fixture(scope="module")
def table(rec):
    t = np.random.default_rng(12).integers(0, 256, (256, 3)).astype(np.uint8)
    rec.set_colormap(t)
    return t


@pytest.fixture(scope="module")
def capped_db():
    """(2, 1025, 1024): 1 049 600 pixels per B-scan want 257 parts and get 256, so every part strides.  B-scan 0 has its minimum in
    the first pixel and its maximum in the last, B-scan 1 both among its final 4096: a lost tail changes the whole picture."""
    rows = DISP_MAX_PARTS * DISP_PART_PIXELS // 1024 + 1
    db = np.random.default_rng(13).uniform(-20.0, 40.0, (2, rows, 1024)).astype(np.float32)
    assert rows * 1024 > DISP_MAX_PARTS * DISP_PART_PIXELS
    db[0, 0, 0], db[0, -1, -1] = -28.0, 60.0
    db[1, -3, 100], db[1, -1, -2] = -28.0, 60.0
    return db


@pytest.mark.parametrize("clamp", [False, True])
def test_display_beyond_the_part_cap(rec, table, capped_db, clamp):
    _check_display(rec, capped_db, -30.0, clamp, table, with_oracle=True)


class _Canaried:
    """A device buffer of n bytes at `offset` bytes behind a 16-byte boundary, 0xA5 on both sides of it."""
    GUARD = 32

    def __init__(self, torch, n, offset):
        self.n, self.at = n, self.GUARD + offset
        self.t = torch.full((self.GUARD + offset + n + self.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.at

    def result(self):
        a = self.t.cpu().numpy()
        assert (a[:self.at] == 0xA5).all() and (a[self.at + self.n:] == 0xA5).all(), "bytes outside the output were written"
        assert (a[self.at - 16:self.at] == 0xA5).all() and (a[self.at + self.n:self.at + self.n + 16] == 0xA5).all()
        return a[self.at:self.at + self.n]


@pytest.mark.parametrize("which", ["aligned", "src", "gray", "bgr", "all"])
def test_display_with_misaligned_device_pointers(rec, table, which):
    """count % 4 == 0, so only the pointers decide between the 16-byte path and the per-pixel one: the source off by one float,
    the grey and the B,G,R output off by one byte, each alone and all together, equal the aligned call and the model, and
    leave the 16 bytes in front of and behind each output alone."""
    import torch
    shape = (2, 64, 40)
    total = 2 * 64 * 40
    db = np.random.default_rng(14).uniform(-60.0, 30.0, shape).astype(np.float32)
    want_gray = np.stack([fm.display(x, -25.0, True) for x in db])
    want_bgr = fm.lut(want_gray, table)
    soff = 1 if which in ("src", "all") else 0
    d_src = torch.zeros(total + 4, dtype=torch.float32, device="cuda")
    d_src[soff:soff + total] = torch.from_numpy(db.reshape(-1)).cuda()
    assert d_src.data_ptr() % 16 == 0
    gray = _Canaried(torch, total, 1 if which in ("gray", "all") else 0)
    bgr = _Canaried(torch, 3 * total, 1 if which in ("bgr", "all") else 0)
    torch.cuda.synchronize()
    rec.display_device(d_src.data_ptr() + 4 * soff, 2, 64, 40, gray.ptr, bgr.ptr, -25.0, True)
    rec.synchronize()
    np.testing.assert_array_equal(gray.result().reshape(shape), want_gray)
    np.testing.assert_array_equal(bgr.result().reshape(shape + (3,)), want_bgr)
    g2, c2 = rec.display(db, -25.0, True, colour=True)                # the aligned call
    np.testing.assert_array_equal(g2, want_gray)
    np.testing.assert_array_equal(c2, want_bgr)


@pytest.mark.parametrize("nbscans", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (1, 3), (1, 5), (1, 7), (3, 85)])
def test_display_of_fewer_pixels_than_lanes(rec, table, nbscans, shape):
    """Most lanes keep their +-1e300 sentinels; 3 x 85 = 255 pixels leave the last wave partly idle and the last quad short."""
    db = np.random.default_rng(15 + shape[1]).uniform(-60.0, 30.0, (nbscans,) + shape).astype(np.float32)
    for thr in (-30.0, -1e9):
        gray, _ = _check_display(rec, db, thr, False, table, with_oracle=True)
        np.testing.assert_array_equal(rec.display(db, thr), gray)
    if shape == (1, 1):
        assert not gray.any()


def test_display_degenerate_ranges(rec, table):
    db = np.random.default_rng(16).uniform(-100.0, -40.0, (2, 6, 6)).astype(np.float32)
    gray, _ = _check_display(rec, db, -30.0, False, table)     # threshold above every pixel: range 0 => scale 0 => zeros
    assert not gray.any()
    gray, _ = _check_display(rec, db, -30.0, True, table)      # ... but (5,5) <- 50: that pixel alone at 255
    want = np.zeros((2, 6, 6), np.uint8)
    want[:, 5, 5] = 255
    np.testing.assert_array_equal(gray, want)
    db = np.random.default_rng(17).uniform(-60.0, 30.0, (2, 9, 13)).astype(np.float32)
    db[0, ::2, ::3] = -np.inf                                  # -inf pixels read as the (finite) threshold
    db[1] = -np.inf
    gray, _ = _check_display(rec, db, -30.0, False, table, with_oracle=True)
    assert gray[0].max() == 255 and not gray[1].any()


def test_display_colour_output_alone(rec, table):
    """A call that asks for the B,G,R image only (gray null) writes what the colour half of a call for both writes."""
    import torch
    for shape in ((2, 64, 40), (3, 3, 85)):
        db = np.random.default_rng(18).uniform(-60.0, 30.0, shape).astype(np.float32)
        _, want = rec.display(db, -30.0, False, colour=True)
        d_db = torch.from_numpy(db).cuda()
        bgr = _Canaried(torch, 3 * db.size, 0)
        torch.cuda.synchronize()
        rec.display_device(d_db.data_ptr(), shape[0], shape[1], shape[2], None, bgr.ptr, -30.0, False)
        rec.synchronize()
        np.testing.assert_array_equal(bgr.result().reshape(shape + (3,)), want)
        np.testing.assert_array_equal(want, fm.lut(np.stack([fm.display(x, -30.0) for x in db]), table))


# ------------------------------------------------------------------------------------------------------------- lock-in

def _lockin_inputs():
    rng = np.random.default_rng(19)
    b = np.abs(rng.standard_normal((3, 33, 7))).astype(np.float32)
    j = np.abs(rng.standard_normal((33, 7))).astype(np.float32)
    b[1, 4] = j[4]                                               # b == j as well as b < j
    return b, j


def _check_lockin(got, b, j):
    np.testing.assert_allclose(got, fm.lockin(b, j), rtol=2e-7, atol=1e-5)   # test_display_chain_bit_exact_and_lockin's figures
    floor = np.broadcast_to(b <= j, b.shape)
    assert floor.any() and np.all(got[floor] == fm.LOCKIN_FLOOR)


def test_lockin_broadcasts_one_jscan_over_an_odd_count(rec):
    """(3, 33, 7): 231 pixels per B-scan, no multiple of 4, the J-scan read again for each of the three."""
    b, j = _lockin_inputs()
    _check_lockin(rec.lockin_db(b, j), b, j)


def test_lockin_device_pointers_off_by_one_float(rec):
    import torch
    b, j = _lockin_inputs()
    d_b = torch.zeros(b.size + 4, dtype=torch.float32, device="cuda")
    d_b[1:1 + b.size] = torch.from_numpy(b.reshape(-1)).cuda()
    d_j = torch.from_numpy(j).cuda()
    out = _Canaried(torch, 4 * b.size, 0)
    torch.cuda.synchronize()
    rec._check(rec.lib.fdoct_lockin_db(rec.h, d_b.data_ptr() + 4, d_j.data_ptr(), capi.MEM_DEVICE, 3, j.size, out.ptr))
    rec.synchronize()
    _check_lockin(out.result().view(np.float32).reshape(b.shape), b, j)
