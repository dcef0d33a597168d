"""The specification of the colour front end (include/fdoct_colour.h; BscanFFTwebcam.cpp:1015-1038 and the block behind it)
in numpy.  Frames are uint8 arrays (..., raw_h, raw_w, 3), B,G,R interleaved as cv::VideoCapture::read delivers them.

  channelnum 0, 1, 2   mraw = that channel, CV_8U: medianBlur and resize(INTER_AREA) as oracle_lib restates them.
  channelnum 3         mraw = (double(B) + double(G) + double(R)) * 0.00130718954, CV_64F: no median (cv::medianBlur rejects
                       CV_64F); resize(INTER_AREA) on doubles in one of two modes:
      "reference"  the block's values added in double from 0.0, rows outermost and left to right, times (double)(1.f / area):
                   ResizeAreaFast as DESIGN.md 3.4c reads it.  What the library computes, bit for bit.
      "truth"      the block's integer B + G + R sums added exactly, one multiplication by the constant and one division by
                   the area in numpy.longdouble, rounded to double once."""
import numpy as np

import oracle_lib

SUM_SCALE = 0.00130718954  # webcam:1031, the literal (1 / 765 = 0.0013071895424...)
MEDIANS = (0, 3, 5, 7)


def _frames(bgr):
    a = np.asarray(bgr)
    assert a.dtype == np.uint8 and a.ndim >= 3 and a.shape[-1] == 3, "frames are (..., raw_h, raw_w, 3) uint8"
    return a.reshape((-1,) + a.shape[-3:]), a.shape[:-3]


def channel_sum(bgr):
    """webcam:1027-1031 on one batch: float64, every value one rounding away from (b + g + r) * SUM_SCALE."""
    a = np.asarray(bgr)
    s = a[..., 0].astype(np.int64) + a[..., 1] + a[..., 2]
    return s.astype(np.float64) * SUM_SCALE


def area_f64(v, binx, biny, mode="reference"):
    """INTER_AREA at integer factors on one float64 picture, block sums rows outermost and left to right."""
    H, W = v.shape
    assert H % biny == 0 and W % binx == 0
    acc = np.zeros((H // biny, W // binx), np.float64)
    for dy in range(biny):
        for dx in range(binx):
            acc = acc + v[dy::biny, dx::binx]
    assert mode == "reference"
    return acc * float(np.float32(1) / np.float32(binx * biny))


def sum_truth(frame, binx, biny):
    """One frame's binned channel sum from exact integers: float64, rounded once from longdouble."""
    s = frame[..., 0].astype(np.int64) + frame[..., 1] + frame[..., 2]
    H, W = s.shape
    assert H % biny == 0 and W % binx == 0
    block = s.reshape(H // biny, biny, W // binx, binx).sum(axis=(1, 3))
    ld = np.longdouble
    return (block.astype(ld) * ld(SUM_SCALE) / ld(binx * biny)).astype(np.float64)


def extract(bgr, channelnum, mediann=0, binx=1, biny=1, mode="reference"):
    """What fdoct_colour_extract writes: uint8 (channelnum 0-2) or float64 (3) of shape (..., raw_h / biny, raw_w / binx)."""
    assert channelnum in (0, 1, 2, 3) and mediann in MEDIANS and binx >= 1 and biny >= 1
    f, lead = _frames(bgr)
    n, H, W, _ = f.shape
    assert H % biny == 0 and W % binx == 0
    if channelnum == 3:
        assert mediann == 0, "cv::medianBlur rejects CV_64F"
        if mode == "truth":
            out = np.stack([sum_truth(x, binx, biny) for x in f])
        elif binx == 1 and biny == 1:
            out = channel_sum(f)
        else:
            out = np.stack([area_f64(channel_sum(x), binx, biny) for x in f])
        return out.reshape(lead + out.shape[1:])
    out = np.empty((n, H // biny, W // binx), np.uint8)
    for i in range(n):
        m = f[i, :, :, channelnum]
        if mediann:
            m = oracle_lib.median_blur(m, mediann)
        m = oracle_lib.resize_area(m, binx, biny)
        assert m.max(initial=0) <= 255
        out[i] = m.astype(np.uint8)
    return out.reshape(lead + out.shape[1:])


def ulps(got, want):
    """|got - want| in units of the spacing of `want`'s doubles."""
    return np.abs(got - want) / np.spacing(np.abs(want))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)
