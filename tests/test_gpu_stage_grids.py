"""GPU tests of the side-stage kernels beyond one pass of their capped grids: the reference-frame capture and the per-frame
min / max (fdoct_capture.hip), lpfilter (fdoct_lowpass.hip), the output binning (fdoct_bscanbin.hip), the colour front end
(fdoct_colour.hip) and the B-scan readouts (fdoct_roi.hip).  Each of these kernels caps its grid -- at resident_blocks(CUs, 16
waves per CU, 256) workgroups, the colour kernels at 8192 -- and walks the rest of its work in a stride loop; the stages' own
test files stay within one pass of those loops.  The cases here are sized from the card's CU count by tests/stage_grid_sizes.py
(held to their conditions on the CPU by tests/test_stage_grid_sizes.py), and every test asserts the inequality that puts it
beyond the cap before it runs anything.

No model and no tolerance of its own: every comparison is the one the stage's test file makes -- bit for bit for the capture,
min / max, colour, holds and A-scan extremes, lowpass_model.parity for the filter, bscanbin_model.parity for the binning,
rtol 1e-12 for the ROI mean.  The readout cases also poison every pixel the reference does not read, so that a mask that lets
one neighbour in shows whatever the data.

On an MI355X (256 CUs: 1024 resident workgroups, 4096 waves, 262 144 threads) the cases are: capture 3122 rows of 126 runs =
393 372 runs, 1.501 passes; min / max one frame of 200 x 126 runs in 99 partials, and 1061 frames of 8 x 40; lowpass 1539
rows; binning 256 images of 3 x 2 tiles = 1536 tiles; colour 3.6 million pixels (1.717 passes of 2 097 152) and 2.25 million
groups of 16 (1.073 passes: the case is sized by its 108 MB of B,G,R, one pass and a partial second one); holds 4397 and 4395
runs over 4096 waves (the image is 16 CUs + 300 A-scans wide: 300 runs into the second pass); A-scan extremes 6147 B-scans;
ROI mean 1539 B-scans.  The module's 76 cases took 7.1 s there: 2.4 s the first capture case, which makes the six u8 frames
its type's cases share, 0.6 s and 0.3 s the lowpass batches of 5850 and 2570 columns, 0.25 s or less every other case."""
import numpy as np
import pytest

import capture_model
import colour_model
import roi_model
import stage_grid_sizes as s
from capture_model import BACKGROUND, PI
from fdoct_amd import Config, Reconstructor, capi
from lowpass_model import lpfilter_truth
from test_gpu_bscanbin import _noise, _parity, _run
from test_gpu_capture import DTYPES, _DeviceFrames, _frames
from test_gpu_colour import _Device, _device_out
from test_gpu_lowpass import _DeviceRows, _every_way, _holds, _input, _same
from test_gpu_roi import _check_slot, _hold, _in_layout, _pictures

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
POISON = np.float32(3e38)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _small_rec(**kw):
    return Reconstructor(Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128, **kw))


def _pad16(W, dtype):
    """Samples that pad a row of W to a pitch of whole 16-byte words."""
    es = np.dtype(dtype).itemsize
    return (-W * es % 16) // es


# ---- 1. capture_accumulate_kernel in a second stride ---------------------------------------------------------------------------
_CAPTURE = {}


def _capture_case(dt):
    """(H, W, runs, six frames, expected values by (role, movavgn)) of one sample type: made once, shared by its cases, and
    dropped when the next type's are made."""
    if dt not in _CAPTURE:
        _CAPTURE.clear()
        H, W, runs = s.capture_shape(dt, _cus())
        frames = np.concatenate([_frames(DTYPES[dt], 1, H, W, seed=300 + i) for i in range(6)])
        frames.setflags(write=False)
        _CAPTURE[dt] = (H, W, runs, frames, {})
    return _CAPTURE[dt]


def _capture_want(case, role, mov):
    frames, wants = case[3], case[4]
    if (role, mov) not in wants:
        fr = frames if role == BACKGROUND else frames[2:3]
        wants[(role, mov)] = capture_model.capture(role, fr, rowwisenormalize=0, donotnormalize=1, movavgn=mov)
    return wants[(role, mov)]


CAPTURE_CASES = [(dt, path) for dt in DTYPES for path in ("aligned", "offset") + (("movavg",) if dt in ("u16", "f64") else ())]


@pytest.mark.parametrize("dt,path", CAPTURE_CASES, ids=["%s-%s" % c for c in CAPTURE_CASES])
def test_capture_beyond_one_pass_of_the_grid(dt, path):
    """Rows of 125 whole 16-byte runs and a tail, enough of them for one and a half passes of the capped grid and a partial
    workgroup.  aligned: a 16-byte aligned pointer and pitch without a moving average -- the 16-byte loads, CAP_INFLIGHT frames
    at a time and a remainder (BACKGROUND from 6 frames) and the start from the first frame's value (PI from one); offset: the
    same frames one sample past a 16-byte boundary, sample by sample; movavg: movavgn 3 on the aligned frames."""
    cus = _cus()
    case = _capture_case(dt)
    H, W, runs, frames = case[:4]
    stride = s.capture_stride(cus)
    assert runs == H * -(-W // s.CAPTURE_RUN[dt]) and s.beyond(runs, stride) and runs % s.BLOCK != 0
    print("capture %s %s: %d CUs, %d x %d samples, %d runs = %.3f passes of %d threads" % (dt, path, cus, H, W, runs, runs / stride, stride))
    mov = 3 if path == "movavg" else 0
    pad, offset = _pad16(W, DTYPES[dt]), int(path == "offset")
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=2048, numdisplaypoints=1024, rowwisenormalize=0, donotnormalize=1,
                               movavgn=mov))
    for role, fr in ((BACKGROUND, frames), (PI, frames[2:3])):
        d = _DeviceFrames(fr, pad, offset)
        assert d.pitch % 16 == 0 and (d.ptr % 16 == 0) == (offset == 0)
        got = rec.capture_reference_device(role, d.ptr, d.dtype, d.n, d.pitch, out=True)
        _same(got, _capture_want(case, role, mov), "role %d" % role)
    rec.close()


# ---- 2. frame_minmax: the fold's second stride, and more frames than workgroups ---------------------------------------------------
def _minmax_device(rec, frames, pad, offset):
    import torch
    d = _DeviceFrames(frames, pad, offset)
    res = torch.zeros(2 * d.n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rec.frame_minmax_device(d.ptr, d.dtype, d.n, d.pitch, res.data_ptr(), res.data_ptr() + 8 * d.n)
    rec.synchronize()
    return res[:d.n].cpu().numpy(), res[d.n:].cpu().numpy()


@pytest.mark.parametrize("dt", ["u16", "f64"])
def test_one_large_frame_takes_the_folds_second_stride(dt):
    """One frame of more than 64 x 256 runs: more than 64 partials, so the fold wave's lane loop strides.  The maximum is the
    frame's last sample; the minimum lies in a run whose workgroup's partial is read in the second stride."""
    cus = _cus()
    H, W, nblk = s.minmax_one_frame(dt, cus)
    V = s.CAPTURE_RUN[dt]
    cpr = -(-W // V)
    assert nblk == s.minmax_blocks(H * cpr, 1, cus) and nblk > 64 and s.beyond(nblk, 64)
    run = s.BLOCK * (nblk - 2) + 17
    assert run < H * cpr and s.minmax_owner(run, nblk) == nblk - 2 >= 64
    print("frame_minmax %s: %d CUs, %d x %d samples, %d partials, minimum in workgroup %d" % (dt, cus, H, W, nblk, nblk - 2))
    frames = _frames(DTYPES[dt], 1, H, W, seed=61)
    lo, hi = (1, 65535) if dt == "u16" else (-1e6, 1e9)
    frames = np.clip(frames, 5, 60000)
    frames[0, run // cpr, (run % cpr) * V] = lo
    frames[0, H - 1, W - 1] = hi
    want_lo, want_hi = capture_model.frame_minmax(frames)
    assert want_lo[0] == lo and want_hi[0] == hi
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=2048, numdisplaypoints=1024))
    for pad, offset in ((_pad16(W, frames.dtype), 0), (3, 1)):   # the 16-byte loads, and sample by sample
        got_lo, got_hi = _minmax_device(rec, frames, pad, offset)
        _same(got_lo, want_lo, "min, offset %d" % offset)
        _same(got_hi, want_hi, "max, offset %d" % offset)
    rec.close()


@pytest.mark.parametrize("dt", ["u16", "u8"])
def test_more_frames_than_workgroups(dt):
    """resident + 37 frames of 8 x 40 samples: every frame's share of the grid is one workgroup, and the fold kernel has more
    waves than one workgroup holds.  Each frame's extremes lie where its index puts them."""
    cus = _cus()
    n, H, W = s.minmax_many_frames(cus), 8, 40
    assert n > s.resident(cus) and s.minmax_blocks(H * -(-W // s.CAPTURE_RUN[dt]), n, cus) == 1 and n > s.WAVES_PER_BLOCK
    print("frame_minmax %s: %d CUs, %d frames of %d x %d" % (dt, cus, n, H, W))
    frames = np.random.default_rng(62).integers(10, 200, (n, H * W)).astype(DTYPES[dt])
    i = np.arange(n)
    p, q = (7 * i) % (H * W), (11 * i + 5) % (H * W)
    q = np.where(q == p, (q + 1) % (H * W), q)
    frames[i, p] = i % 10
    frames[i, q] = 200 + i % 50
    frames = frames.reshape(n, H, W)
    want_lo, want_hi = capture_model.frame_minmax(frames)
    assert np.array_equal(want_lo, i % 10) and np.array_equal(want_hi, 200 + i % 50)
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=1024, numdisplaypoints=512))
    for pad, offset in ((_pad16(W, frames.dtype), 0), (3, 1)):
        got_lo, got_hi = _minmax_device(rec, frames, pad, offset)
        _same(got_lo, want_lo, "min, offset %d" % offset)
        _same(got_hi, want_hi, "max, offset %d" % offset)
    rec.close()


# ---- 3. lowpass_rows_kernel: more rows than workgroups, and the widths between the tested ones ------------------------------------
@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=128, height=96, numfftpoints=1024, numdisplaypoints=512))
    yield r
    r.close()


@pytest.mark.parametrize("W", s.LOWPASS_BATCH_WIDTHS)
def test_lowpass_more_rows_than_workgroups(rec, W):
    """One and a half passes of the row loop and three rows: a workgroup's second row reuses xs / part / Fs (or its slice of
    the workspace) behind the loop's last barrier.  128: staged, 8 slices; 2570: staged, 257 bins; 5850: bins in the workspace;
    9: no bin at all, the `continue` in front of every barrier; 1: the copy."""
    cus = _cus()
    rows = s.lowpass_rows(cus)
    assert s.beyond(rows, s.resident(cus))
    f, G, _, _, staged = s.lowpass_shape(W)
    assert (f, G, staged) == s.LOWPASS_EXPECT[W]
    print("lowpass W %d: %d CUs, %d rows over %d workgroups, f %d G %d staged %d" % (W, cus, rows, s.resident(cus), f, G, staged))
    x = _input("noise", rows, W, seed=700 + W)
    d = _DeviceRows(x)
    rec.lowpass_rows_device(d.ptr, rows, W)
    rec.synchronize()
    first = d.host().copy()
    _holds(first, x, "%d x %d, device, packed, in place" % (rows, W))
    if W == 1:
        _same(first, x, "W = 1 blanks nothing")
    elif W < 10:
        assert np.all(first == 0.0)
    src, dst = _DeviceRows(x, pad=3), _DeviceRows(np.zeros_like(x), pad=3)
    rec.lowpass_rows_device(src.ptr, rows, W, src.pitch, dst.ptr)
    rec.synchronize()
    _same(src.host(), x, "the input of an out-of-place call changed")
    _same(dst.host(), first, "device, padded, out of place")
    r = s.resident(cus) + 5                                  # a row of the second pass, alone: some workgroup's first row
    one = _DeviceRows(x[r:r + 1])
    rec.lowpass_rows_device(one.ptr, 1, W)
    rec.synchronize()
    _same(one.host(), first[r:r + 1], "row %d alone and in the batch" % r)


@pytest.mark.parametrize("kind", ["normalised", "noise"])
@pytest.mark.parametrize("W", s.LOWPASS_WIDTHS)
def test_lowpass_widths_between_the_tested_ones(rec, W, kind):
    """369, 400, 519, 850: 7, 6, 5 and 3 slices a bin.  2570 .. 5849: more than 256 bins staged in LDS -- the analysis loop's
    second stride and the synthesis' re-seeded phasor; 5849 fills the 64 KB to the byte, 5850 is the first width whose bins
    live in the workspace."""
    f, G, _, lds, staged = s.lowpass_shape(W)
    assert (f, G, staged) == s.LOWPASS_EXPECT[W]
    if W == 5849:
        assert lds == 65536
    for rows in (1, 5):
        x = _input(kind, rows, W, seed=rows + W)
        truth = lpfilter_truth(x)
        first = None
        for what, got in _every_way(rec, x):
            if first is None:
                first = got
                _holds(got, x, "%d x %d %s, %s" % (rows, W, kind, what), truth)
            else:
                _same(got, first, what)


# ---- 4. bscan_bin_kernel: more tiles than workgroups --------------------------------------------------------------------------
def _bin_case(f, layout, quad, cus):
    """Pictures (n, D, H) whose output has bin_tiles(cus) tiles in memory, the last one of either direction partial."""
    binx, biny, upx, upy = f
    upr, upc = (upy, upx) if layout == TR else (upx, upy)     # memory rows are depths in the transposed layout, A-scans otherwise
    rows, cols = s.bin_output(cus, upr, upc, quad)
    od, oa = (rows, cols) if layout == TR else (cols, rows)
    D, H = od // upy * biny, oa // upx * binx
    assert capi.bscanbin_size(D, H, binx, biny, upx, upy) == (od, oa)
    n = s.bin_images(cus)
    pics = _noise(n, D, H, 800 + D + H)
    g = np.arange(n)
    pics[g, (5 * g + 3) % D, (7 * g + 1) % H] += 4000.0       # one spike per image, where its index puts it
    return pics, rows, cols


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("quad", [False, True], ids=["odd", "quad"])
@pytest.mark.parametrize("f", [(1, 1, 1, 1), (2, 2, 2, 2), (3, 1, 3, 1)])
def test_binning_more_tiles_than_workgroups(f, quad, layout):
    """Small images of 3 x 2 tiles, as many as give one and a half passes of the tile loop: a workgroup's second tile lies at
    another position of another image than its first (6 does not divide the grid), behind the loop-top barrier.  odd: a column
    count that is no multiple of 4, element by element; quad: the 16-byte loads and stores.  The DC mask is on."""
    cus = _cus()
    tr, tc = s.bin_tiles(cus)
    pics, rows, cols = _bin_case(f, layout, quad, cus)
    n = pics.shape[0]
    assert -(-rows // s.BIN_TILE_R) == tr and -(-cols // s.BIN_TILE_C) == tc and rows % s.BIN_TILE_R and cols % s.BIN_TILE_C
    assert s.resident(cus) % (tr * tc) != 0 and s.beyond(n * tr * tc, s.resident(cus)) and (cols % 4 == 0) == quad
    print("binning %s: %d CUs, %d images of %d x %d outputs (memory), %d tiles over %d workgroups" %
          (f, cus, n, rows, cols, n * tr * tc, s.resident(cus)))
    rec = _small_rec()
    lin, db = _run(rec, pics, layout, True, f)
    _parity(lin, db, pics, f, "tile loop")
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
def test_binning_more_tiles_than_workgroups_behind_the_lock_in(layout):
    """The same with jscan (the lock-in's difference in front of the sums; no DC mask then)."""
    cus = _cus()
    f = (2, 2, 2, 2)
    tr, tc = s.bin_tiles(cus)
    pics, rows, cols = _bin_case(f, layout, False, cus)
    assert s.resident(cus) % (tr * tc) != 0 and s.beyond(pics.shape[0] * tr * tc, s.resident(cus))
    jscan = _noise(1, pics.shape[1], pics.shape[2], 9)[0] * np.float32(0.5)
    rec = _small_rec()
    lin, db = _run(rec, pics, layout, True, f, jscan=jscan)
    _parity(lin, db, pics, f, "tile loop, jscan", jscan=jscan)
    rec.close()


# ---- 5. colour_px_kernel and colour_vec_kernel beyond 8192 workgroups -------------------------------------------------------------
def _colour_case(rec, out_shape, bins, c, pad, offset, seed):
    n, oh, ow = out_shape
    h, w = oh * bins[1], ow * bins[0]
    f = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    d = _Device(f, row_bytes=3 * w, pad=pad, offset=offset)
    want = colour_model.extract(f, c, 0, *bins)
    out, read = _device_out(want.shape, want.dtype)
    rec.colour_extract_device(d.ptr, n, w, h, d.pitch, c, out.data_ptr(), 0, *bins)
    rec.synchronize()
    got = read()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(colour_model.bits(got), colour_model.bits(want))
    return d


@pytest.mark.parametrize("bins", [(1, 1), (2, 2), (3, 1)])
@pytest.mark.parametrize("c", [1, 3])
def test_colour_pixel_kernel_beyond_one_pass(c, bins):
    """Frames one byte past a 16-byte boundary: every output pixel is colour_px_kernel's, 3.6 million of them."""
    n, oh, ow = s.COLOUR_PX_OUT
    items = s.colour_px_items()
    assert items == n * oh * ow and s.beyond(items, s.COLOUR_STRIDE)
    print("colour px c %d bins %s: %d output pixels = %.3f passes of %d" % (c, bins, items, items / s.COLOUR_STRIDE, s.COLOUR_STRIDE))
    rec = _small_rec()
    d = _colour_case(rec, s.COLOUR_PX_OUT, bins, c, pad=0, offset=1, seed=90 + c)
    assert d.ptr % 16 == 1                                    # colour_vectorised is false
    rec.close()


def test_colour_vector_kernel_beyond_one_pass():
    """Aligned frames of 16 x 125 + 5 columns, 36 million output pixels: 2.25 million groups of 16 for colour_vec_kernel (one
    pass of 8192 workgroups and a partial second one) and the 5 columns a row leaves over for colour_px_kernel."""
    n, oh, ow = s.COLOUR_VEC_OUT
    items = s.colour_vec_items()
    assert items == n * oh * (ow // 16) and items > s.COLOUR_STRIDE + s.COLOUR_STRIDE // 16 and items % s.COLOUR_STRIDE != 0 and ow % 16 == 5
    print("colour vec: %d groups of 16 = %.3f passes of %d" % (items, items / s.COLOUR_STRIDE, s.COLOUR_STRIDE))
    rec = _small_rec()
    d = _colour_case(rec, s.COLOUR_VEC_OUT, (1, 1), 1, pad=(-3 * ow) % 16, offset=0, seed=95)
    assert d.ptr % 16 == 0 and d.pitch % 16 == 0              # colour_vectorised is true
    rec.close()


# ---- 6. the readouts: second strides, and masks against poisoned surroundings ----------------------------------------------------
def _poisoned(pics, roi):
    """The pictures with +3e38 in every pixel printPeakHoldAscan does not read: all but ROI rows y .. y + h - 1 in columns
    x .. x + w - 1 and in column ascanat."""
    x, y, w, h, ascanat = roi
    p = np.full(pics.shape, POISON, np.float32)
    p[:, y:y + h, x:x + w] = pics[:, y:y + h, x:x + w]
    p[:, y:y + h, ascanat] = pics[:, y:y + h, ascanat]
    return p


def _hold_and_check(rec, model, roi, pics, layout, offset=0):
    rec.set_peakhold_roi(*roi)
    model.set_roi(*roi)
    rec.clear_peakhold(1)
    model.clear(1)
    _hold(rec, 1, pics, layout, True, offset)
    model.fold(1, pics)
    _check_slot(rec, model, 1)
    cols, amax, _ = rec.peakhold_values(1)
    assert cols.max() < 1e38 and amax < 1e38, "a pixel outside the ROI was read"


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("D,offset", [(12, 0), (9, 0), (12, 1)], ids=["quads", "D9", "misaligned"])
def test_hold_of_more_runs_than_waves(D, offset, layout):
    """16 CUs + 300 A-scans: in the row-major layout an ROI that wide has more runs (w + 1) than the grid has waves, so the
    kernel's wave loop takes a second item.  D = 12 on a 16-byte aligned image takes the 16-byte loads; D = 9, and D = 12 behind
    a 4-byte offset, the element loads.  The transposed layout folds the same images (its items are chunks of 64 lanes across
    the ROI, far fewer than waves)."""
    cus = _cus()
    H, nb = s.hold_ascans(cus), 3
    pics = _pictures(nb, D, H, 70 + D)
    rec, model = _small_rec(), roi_model.PeakHold()
    for roi in [(0, 0, H, D, H - 1), (1, 1, H - 2, D - 2, H // 2)]:    # the whole image; one pixel in from every border
        x, y, w, h, _ = roi
        if layout == ROW:
            vec = offset == 0 and D % 4 == 0
            items, slices = s.hold_items(w, nb, ((y + h + 3) >> 2) - (y >> 2) if vec else h, cus)
            assert slices == 1 and items == w + 1 > s.roi_waves(cus)
            print("hold D %d offset %d: %d CUs, %d runs over %d waves" % (D, offset, cus, items, s.roi_waves(cus)))
        _hold_and_check(rec, model, roi, _poisoned(pics, roi), layout, offset)
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
def test_hold_masks_against_poisoned_surroundings(layout):
    """Every combination of (first mod 4, end mod 4) of the ROI's edges along the contiguous dimension of a 16-byte aligned
    image whose rows are whole quads -- depths in the row-major layout, A-scans in the transposed one -- with ROIs shorter than
    a quad (one pixel among them) and longer ones; everything the reference does not read is +3e38."""
    n, L, S = 2, 16, 7                                        # L along the quads, S across
    D, H = (L, S) if layout == ROW else (S, L)
    pics = _pictures(n, D, H, 75, loc=5.0)
    assert (pics < 0).any() and (pics > 0).any()
    rec, model = _small_rec(), roi_model.PeakHold()
    seen = set()
    for a in range(4):
        for b in range(4):
            first = 4 + a
            short = (b - first) % 4 or 4
            for length, across in ((short, (3, 1, 5)), (short + 4, (1, S - 2, 0)), (short + 4, (2, 3, 3))):
                lo, ext, ascanat = across
                if layout == ROW:
                    roi = (lo, first, ext, length, ascanat)
                else:
                    roi = (first, lo, length, ext, (first + 1) % H if ascanat else 0)
                seen.add((first % 4, (first + length) % 4))
                _hold_and_check(rec, model, roi, _poisoned(pics, roi), layout)
    assert len(seen) == 16
    roi = (3, 9, 1, 1, 5) if layout == ROW else (9, 3, 1, 1, 0)        # one pixel
    _hold_and_check(rec, model, roi, _poisoned(pics, roi), layout)
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("D", [9, 8])
def test_ascan_minmax_of_more_bscans_than_waves(D, layout):
    """One and a half passes of the wave-per-B-scan loop; D = 8 in the row-major layout reads quads.  Depth rows 0-3 carry
    +-500 and every other A-scan +-3e38: neither may count."""
    import torch
    cus = _cus()
    nb, H = s.minmax_bscans(cus), 3
    assert s.beyond(nb, s.roi_waves(cus))
    print("ascan_minmax D %d: %d CUs, %d B-scans over %d waves" % (D, cus, nb, s.roi_waves(cus)))
    pics = _pictures(nb, D, H, 31 + D)
    sign = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None, None]
    pics[:, 0:4, :] += 500.0 * sign
    rec = _small_rec()
    for ascanat in range(H):
        p = np.broadcast_to(POISON * sign, pics.shape).copy()
        p[:, :, ascanat] = pics[:, :, ascanat]
        t = torch.from_numpy(_in_layout(p, layout)).cuda()
        out = torch.zeros(2 * nb, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert t.data_ptr() % 16 == 0
        rec.ascan_minmax_device(t.data_ptr(), nb, D, H, ascanat, out.data_ptr(), out.data_ptr() + 4 * nb, layout)
        rec.synchronize()
        lo, hi = out[:nb].cpu().numpy(), out[nb:].cpu().numpy()
        mlo, mhi = roi_model.min_max_ascan(p, ascanat)
        np.testing.assert_array_equal(lo, mlo)
        np.testing.assert_array_equal(hi, mhi)
        assert (np.abs(hi) < 400).all() and (np.abs(lo) < 400).all()
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
def test_roi_mean_of_more_bscans_than_workgroups(layout):
    """One and a half passes of the workgroup-per-B-scan loop -- the partial sums in LDS are reused behind the loop's last
    barrier -- with a box of 290 A-scans, two strides of the column loop.  Everything outside the box is 1e30."""
    cus = _cus()
    nb, (D, H), width = s.mean_bscans(cus), s.MEAN_SHAPE, s.MEAN_WIDTH
    assert s.beyond(nb, s.resident(cus)) and s.BLOCK < width < 2 * s.BLOCK
    print("roi_mean: %d CUs, %d B-scans over %d workgroups" % (cus, nb, s.resident(cus)))
    pics = _pictures(nb, D, H, 41)
    rec = _small_rec()
    for ascanat, vertpos in [(0, 0), (9, 2), (4, 1)]:
        p = np.full(pics.shape, 1e30, np.float32)
        p[:, vertpos:vertpos + 3, ascanat:ascanat + width] = pics[:, vertpos:vertpos + 3, ascanat:ascanat + width]
        a = _in_layout(p, layout)
        got = rec.roi_mean(a, ascanat, vertpos, width, layout)
        np.testing.assert_allclose(got, roi_model.avg_roi(p, ascanat, vertpos, width), rtol=1e-12, atol=0)
        assert (np.abs(got) < 100).all()
        np.testing.assert_array_equal(rec.roi_mean(a, ascanat, vertpos, width, layout), got)
    rec.close()
