"""The specification of the per-frame saves while averaging (include/fdoct_saveframes.h) in NumPy, in doubles.

Pictures (BscanFFT.cpp:1360-1377; the manual branch, 1447-1467, starts from images that are D x H already):
  transpose(bscansave[ii], t); t += 0.000001; log(t, t); t = 20.0 * t / 2.303; normalize(t, t, 0, 1, NORM_MINMAX);
  t.convertTo(t, CV_8UC1, 255.0)
on the float magnitudes widened to double: d = 20.0 * ln(x + 0.000001) / 2.303, lo / hi the extrema of d over the image,
scale = 1 / (hi - lo) if hi - lo > DBL_EPSILON else 0, shift = 0 - lo * scale, byte = saturate(rint((d * scale + shift) * 255.0))
-- the normalise and convert frontend_model.display states for fdoct_display, with no threshold and no clamp.  x + 0.000001 is
clamped from below at 0.000001 (a negative input only: cv::log is undefined there).

Fold (BscanFFT.cpp:1197-1240): per group of `averages` frames the sum in double in frame order, b = acc / averages + eps,
bscan = float32(b), bscandb = float32(20.0 * ln(b) / 2.303), and with dc_mask and more than four depth rows depth row 4 of
bscandb over its rows 1 and 0.

Layouts: ROWMAJOR images are (ascans, depths) = H x D, TRANSPOSED ones (depths, ascans) = D x H.  Pictures are always D x H.
"""
import numpy as np

ROWMAJOR, TRANSPOSED = 0, 1
EPS_MAIN = 0.00001   # main:1222, as a double
TILE = 64            # the picture pass's tile on H x D input (fdoct_saveframes.hip): where the shared inputs put their extrema


def db_values(x):
    x = np.asarray(x)
    assert x.dtype == np.float32
    return 20.0 * np.log(np.maximum(x.astype(np.float64) + 0.000001, 0.000001)) / 2.303


def unrounded(frame, in_layout):
    """One image -> (the D x H picture before rint and saturation, lo, hi)."""
    frame = np.asarray(frame)
    assert frame.ndim == 2
    d = db_values(frame)
    if in_layout == ROWMAJOR:
        d = np.ascontiguousarray(d.T)
    lo, hi = d.min(), d.max()
    scale = 1.0 / (hi - lo) if hi - lo > np.finfo(np.float64).eps else 0.0
    shift = 0.0 - lo * scale
    return (d * scale + shift) * 255.0, lo, hi


def image(frame, in_layout):
    """One image of float32 magnitudes -> its save picture, uint8 (depths, ascans)."""
    u, _, _ = unrounded(frame, in_layout)
    return np.clip(np.rint(u), 0, 255).astype(np.uint8)


def fold(frames, averages, eps, dc_mask, in_layout, out_layout):
    """frames float32 (nframes, rows, cols) in in_layout -> (bscan, bscandb) float32 (nframes / averages, ..) in out_layout."""
    a = np.asarray(frames)
    assert a.dtype == np.float32 and a.ndim == 3 and averages >= 1 and a.shape[0] % averages == 0
    bs, dbs = [], []
    for g in range(a.shape[0] // averages):
        acc = np.zeros(a.shape[1:], np.float64)
        for f in range(averages):
            acc = acc + a[g * averages + f].astype(np.float64)     # 1197
        b = acc / float(averages) + eps                             # 1221-1222
        db = 20.0 * np.log(b) / 2.303                               # 1235-1237
        if in_layout == ROWMAJOR:
            b, db = b.T, db.T                                       # 1220: D x H from here on
        db = np.array(db)
        if dc_mask and db.shape[0] > 4:
            db[1] = db[4]                                           # 1239
            db[0] = db[4]                                           # 1240
        if out_layout == ROWMAJOR:
            b, db = b.T, db.T
        bs.append(np.ascontiguousarray(b).astype(np.float32))
        dbs.append(np.ascontiguousarray(db).astype(np.float32))
    return np.array(bs), np.array(dbs)


def tie_band(lo, hi):
    """How far a device value may sit from the model's before rounding: d, lo and hi are each allowed two double ulps, with a
    factor of room."""
    return 255.0 * 16.0 * 2.0 ** -52 * max(abs(lo), abs(hi)) / (hi - lo)


def tie_distance(frame, in_layout):
    """(the smallest distance of an unrounded pixel of the picture from a half-integer, the image's tie band); (inf, 0) for a
    constant image, whose pixels are all exactly 0."""
    u, lo, hi = unrounded(frame, in_layout)
    if not hi - lo > np.finfo(np.float64).eps:
        return np.inf, 0.0
    return float(np.abs(u - np.floor(u) - 0.5).min()), tie_band(lo, hi)


# ---- inputs shared by the CPU and the GPU tests

PICTURE_SHAPES = ((1, 1), (1, 7), (7, 1), (3, 85), (64, 64), (65, 64), (67, 129))   # (H, D)
EXTRA_PICTURE_SETS = (((68, 64), 3), ((16, 12), 3), ((1, 7), 5000))   # (shape, n): the pointer, refusal and many-images tests
BIG_SHAPE = (1025, 1024)   # beyond 256 partial extrema x 4096 pixels per image, and beyond one pass of the capped grids

_FRAMES = {}


def frames_hd(shape, n, first=0):
    """n images (H, D) of lognormal magnitudes (sigma = 4 in ln), read-only and remembered.  Image k has content kind (first + k) % 3:
      0  no zeros but ONE: the minimum sits in the first pixel, the maximum in the last
      1  no zeros but ONE: the minimum sits in the first pixel of the last (partial) tile, the maximum in the last pixel
      2  5 % exact zeros, anywhere
    (images of one pixel are what they are)."""
    key = (tuple(shape), n, first)
    if key not in _FRAMES:
        H, D = shape
        rng = np.random.default_rng(7919 * H + 104729 * D + 31 * n + first)
        a = np.exp(rng.normal(0.0, 4.0, (n, H, D))).astype(np.float32)
        for k in range(n):
            kind, img = (first + k) % 3, a[k]
            if kind == 2 or img.size == 1:
                img[rng.random((H, D)) < 0.05] = 0.0
                continue
            top = np.float32(2.0) * img.max()
            lo_at = (0, 0) if kind == 0 else (TILE * ((H - 1) // TILE), TILE * ((D - 1) // TILE))
            if lo_at == (H - 1, D - 1):
                lo_at = (0, 0)
            img[H - 1, D - 1] = top
            img[lo_at] = 0.0
        a.setflags(write=False)
        _FRAMES[key] = a
    return _FRAMES[key]


def in_layout_of(frames_hd_, in_layout):
    """The (n, H, D) images as the call takes them in in_layout (a contiguous copy for TRANSPOSED)."""
    return frames_hd_ if in_layout == ROWMAJOR else np.ascontiguousarray(np.transpose(frames_hd_, (0, 2, 1)))


def fold_frames(n, H, D, seed=0):
    """n images (H, D) for the fold: uniform(0, 50) with a few exact zeros and exact repeats from image to image."""
    key = ("fold", n, H, D, seed)
    if key not in _FRAMES:
        rng = np.random.default_rng(1000 * seed + 17 * H + D + n)
        a = rng.uniform(0.0, 50.0, (n, H, D)).astype(np.float32)
        a[rng.random((n, H, D)) < 0.02] = 0.0
        for k in range(1, n):
            a[k, k % H, :] = a[k - 1, k % H, :]
        a.setflags(write=False)
        _FRAMES[key] = a
    return _FRAMES[key]
