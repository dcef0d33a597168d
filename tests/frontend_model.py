"""The camera front end (fdoct_generic.hip: median_kernel, median3_fast_kernel, bin_kernel, bin2x2_kernel) and the display
post-chain (fdoct_display.hip) restated in numpy and scipy only: a second statement of the same operations, written without
the kernels' or the oracle's loops, so that a misreading shared by those two shows (tests/test_frontend_model.py holds it to
the oracle on the CPU; tests/test_gpu_frontend_edges.py holds the kernels to it).

  median    cv::medianBlur(ksize n): the n x n median with a replicated border, per frame.
  bin_area  cv::resize(INTER_AREA) at integer factors on 8- / 16-bit samples: the block's integer sum, then (s + 2) >> 2 for
            2 x 2 (round half up) and rint(float32(s) * float32(1 / area)) for every other factor (round half to even).
            Up to binx * biny = 256 an integer and a float32 accumulation of 16-bit samples agree exactly (the sum stays below
            2^24); beyond that area they need not, so the model refuses it for 16-bit frames.
  display   max(db, thr); optionally (5,5) <- 50; min-max normalise to 0..1; x 255 -> u8: every step one float64 numpy
            operation, each rounded once, no fused multiply-add -- the kernel's contract.
  lut       a 256-entry B,G,R table look-up.
  lockin    20 * ln(max(b - j, 0) + 0.001) / 2.303 in float64, narrowed to float32."""
import numpy as np
from scipy import ndimage

MAX_AREA_U16 = 256  # 256 * 65535 < 2^24: the largest area whose 16-bit block sums every float32 holds exactly


def _frames(frames):
    a = np.asarray(frames)
    assert a.dtype in (np.uint8, np.uint16) and a.ndim in (2, 3), "frames are (nframes, h, w) or (h, w), uint8 or uint16"
    return (a[None] if a.ndim == 2 else a), a.ndim == 2


def median(frames, n):
    """n x n median of every frame on its own, border replicated; same dtype and shape."""
    assert n in (3, 5, 7)
    a, single = _frames(frames)
    out = np.stack([ndimage.median_filter(f, size=n, mode="nearest") for f in a])
    return out[0] if single else out


def block_sums(frames, binx, biny):
    """Integer sums of the binx x biny blocks: uint32 (nframes, h / biny, w / binx)."""
    a, _ = _frames(frames)
    n, h, w = a.shape
    assert binx >= 1 and biny >= 1 and h % biny == 0 and w % binx == 0
    assert a.dtype == np.uint8 or binx * biny <= MAX_AREA_U16, "16-bit block sums beyond area 256 do not fit a float32 exactly"
    return a.reshape(n, h // biny, biny, w // binx, binx).sum(axis=(2, 4), dtype=np.uint32)


def bin_area(frames, binx, biny):
    a, single = _frames(frames)
    s = block_sums(a, binx, biny)
    if binx == 2 and biny == 2:
        o = (s + np.uint32(2)) >> np.uint32(2)
    else:
        o = np.rint(s.astype(np.float32) * np.float32(1.0 / (binx * biny)))
    o = o.astype(a.dtype)
    return o[0] if single else o


def frontend(frames, mediann=0, binx=1, biny=1):
    """What Reconstructor.frontend returns: the median (0: none), then the binning."""
    m = median(frames, mediann) if mediann else np.asarray(frames)
    return bin_area(m, binx, biny)


def ties(frames, binx, biny):
    """Where a block sum lies exactly between two output values (even areas only: no sum of integers is half a third)."""
    area = binx * biny
    s = block_sums(frames, binx, biny)
    return (s % area) * 2 == area


def display(db_f32, thr=-30.0, clampupper=False):
    """One B-scan (rows, cols) of float32 dB -> uint8."""
    db = np.asarray(db_f32)
    assert db.dtype == np.float32 and db.ndim == 2
    d = np.maximum(db.astype(np.float64), thr)
    if clampupper:
        d[5, 5] = 50.0
    lo, hi = d.min(), d.max()
    scale = 1.0 / (hi - lo) if hi - lo > np.finfo(float).eps else 0.0
    shift = 0.0 - lo * scale
    return np.clip(np.rint((d * scale + shift) * 255.0), 0, 255).astype(np.uint8)


def lut(gray, table):
    t = np.asarray(table, np.uint8).reshape(256, 3)
    return t[np.asarray(gray, np.uint8)]


def lockin(b, j):
    b64, j64 = np.asarray(b, np.float32).astype(np.float64), np.asarray(j, np.float32).astype(np.float64)
    return (20 * np.log(np.maximum(b64 - j64, 0) + 0.001) / 2.303).astype(np.float32)


LOCKIN_FLOOR = np.float32(20 * np.log(0.001) / 2.303)  # every pixel with b <= j


# ---- frames for the tests (shared by the CPU and the GPU test so that both look at the same cases)

SMALL_SHAPES = ((1, 1), (1, 8), (1, 9), (2, 3), (3, 2), (4, 16), (7, 7))  # (h, w): smaller than a 7 x 7 window, or one tile of it
SMALL_BIN_SHAPE, SMALL_BINS = (4, 6), ((3, 2), (6, 4), (1, 4), (6, 1))     # (h, w); (binx, biny)
TIE_BINS = ((2, 1), (1, 2), (3, 1), (1, 3), (4, 1), (1, 4), (3, 2), (2, 3), (4, 2), (2, 4), (4, 3), (3, 4))  # areas 2 3 4 6 8 12


def small_frames(dtype, h, w, seed=0):
    """3 frames of different content with extremes on the first and last row and column."""
    top = np.iinfo(dtype).max
    rng = np.random.default_rng(1000 * h + w + seed)
    a = rng.integers(0, top + 1, (3, h, w)).astype(dtype)
    a[0, 0, :] = top
    a[0, -1, :] = 0
    a[1, :, 0] = 0
    a[1, :, -1] = top
    a[2] = top - a[2] // 2        # a brighter frame: a row read from a neighbouring frame moves the median
    return a


def tie_frame(dtype, binx, biny, wblocks=8):
    """One frame whose blocks have the sums area * q + area / 2 (area // 2 and area // 2 + 1 for area 3: the nearest thirds) for
    quotients q, even and odd, at the bottom, the middle and the top of the sample range; the block's samples differ where
    they can.  Returns (frame, the quotients per block)."""
    area, top = binx * biny, int(np.iinfo(dtype).max)
    mid = (top + 1) // 2
    qs = [0, 1, 2, 3, mid - 2, mid - 1, mid, mid + 1, top - 4, top - 3, top - 2, top - 1]
    qs = np.array(qs * wblocks).reshape(-1, wblocks)             # one row of blocks per quotient parity / range
    rem = np.full(qs.shape, area // 2)
    if area % 2:
        rem[:, 1::2] += 1
    sums = qs * area + rem
    frame = np.empty((qs.shape[0] * biny, wblocks * binx), np.int64)
    for by in range(qs.shape[0]):
        for bx in range(wblocks):
            # spread the sum unevenly: base everywhere, the remainder one count at a time, then move counts between two samples
            base, extra = divmod(int(sums[by, bx]), area)
            blk = np.full(area, base)
            blk[:extra] += 1
            if area > 1:
                d = min(int(blk[0]), top - int(blk[-1]), 3)
                blk[0] -= d
                blk[-1] += d
            frame[by * biny:(by + 1) * biny, bx * binx:(bx + 1) * binx] = blk.reshape(biny, binx)
    assert frame.min() >= 0 and frame.max() <= top
    return frame.astype(dtype), qs


# 2 x 2 (a tie is s = 4 q + 2 and must go up): blocks per row that make a raw row whole 16-byte vectors, 8- and 16-bit alike
# (bin2x2_kernel), and that do not (bin_kernel's own 2 x 2 branch)
TIE_2X2_WBLOCKS = {"bin2x2_kernel": 8, "bin_kernel": 7}
