"""The reference's key-handler recipe for data_yb / data_yp / data_yd (BscanFFT.cpp:1000-1099, BscanDark.cpp:1005-1190,
BscanFFTsim.cpp:803-825), composed from what tests/oracle_lib.py restates -- medianBlur, INTER_AREA binning, smoothmovavg,
normalizerows, cv::normalize(NORM_MINMAX) -- plus a float64 accumulation in frame order.  The expected value of every
test of include/fdoct_capture.h."""
import numpy as np

import oracle_lib

BACKGROUND, PI, DARK, NONE = range(4)


def front_end(frames, mediann=0, binx=1, biny=1):
    """main:953-958 on every raw frame: medianBlur, then resize(INTER_AREA).  Same dtype out (u8 / u16)."""
    frames = np.asarray(frames)
    if mediann == 0 and binx == 1 and biny == 1:
        return frames
    out = []
    for f in frames:
        g = f.astype(np.uint16)
        if mediann:
            g = oracle_lib.median_blur(g, mediann)
        if binx > 1 or biny > 1:
            g = oracle_lib.resize_area(g, binx, biny)
        out.append(g.astype(frames.dtype))
    return np.stack(out)


def capture(role, frames, rowwisenormalize=0, donotnormalize=1, movavgn=0, sim=False, mediann=0, binx=1, biny=1):
    """float64 (H, W): what the handle holds after the key handler of `role` saw `frames` (nframes, rows, cols)."""
    binned = front_end(frames, mediann, binx, biny)
    if sim and role in (BACKGROUND, PI):            # sim:803-825: the frame itself
        assert len(binned) == 1
        return binned[0].astype(np.float64)
    data_y = [f.astype(np.float64) for f in binned]
    if not sim and movavgn > 0:                     # main:990-991
        data_y = [oracle_lib.smoothmovavg(y, movavgn) for y in data_y]
    if role == PI:                                  # main:1081-1096
        assert len(data_y) == 1
        y = data_y[0].copy()
        if rowwisenormalize:
            y = oracle_lib.normalizerows(y, 0.0, 1.0)
        if not donotnormalize:
            y = oracle_lib.normalize_minmax(y.ravel(), 0.0, 1.0).reshape(y.shape)
        return y
    acc = np.zeros(data_y[0].shape, np.float64)     # baccum = Mat::zeros, main:1061
    for y in data_y:                                # accumulate(data_y, baccum), main:1043, frame by frame
        acc = acc + y
    if rowwisenormalize:                            # main:1050-1057
        acc = oracle_lib.normalizerows(acc, 0.0001, 1.0)
    if not donotnormalize:
        acc = oracle_lib.normalize_minmax(acc.ravel(), 0.0001, 1.0).reshape(acc.shape)
    else:
        acc = acc / float(len(data_y))
    return acc


def frame_minmax(frames, mediann=0, binx=1, biny=1):
    """main:1105-1108 per frame: minMaxLoc of the binned frame."""
    b = front_end(frames, mediann, binx, biny).astype(np.float64)
    return b.min(axis=(1, 2)), b.max(axis=(1, 2))


def bits(a):
    """The doubles as uint64 words, so that comparisons count the sign of zero."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
