"""numpy restatement of the reference's B-scan readouts (include/fdoct_roi.h), line by line where it matters for parity.

Images here are in the reference's picture, `bscandb` as a D x H Mat: pictures(n, depths, ascans).  picture() turns a batch
in either of the library's layouts into that form.
"""
import numpy as np

LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED = 0, 1
PI = 3.141592653589793  # BscanFFTpeak.cpp:495

# besseldbinverse, BscanFFTpeak.cpp:243-395: x = BINV_X[i] for the first i with y > BINV_T[i], else 0.0
BINV_T = [30, 25, 21.65, 19.2, 17.18, 15.56, 14.19, 13, 11.94, 11, 10.15, 9.37, 8.66, 8, 7.4, 6.83, 6.30, 5.82, 5.36, 4.931,
          4.528, 4.151, 3.797, 3.464, 3.151, 2.858, 2.583, 2.3245, 2.08286, 1.85689, 1.64601, 1.44964, 1.26729, 1.09850,
          0.94288, 0.80006, 0.66972, 0.55159, 0.44542, 0.35097, 0.26807, 0.19654, 0.13625, 0.08708, 0.04893, 0.02173, 0.00543]
BINV_X = [2.38, 2.33, 2.27, 2.22, 2.17, 2.12, 2.07, 2.02, 1.97, 1.92, 1.87, 1.82, 1.77, 1.72, 1.67, 1.62, 1.57, 1.52, 1.47,
          1.42, 1.37, 1.32, 1.27, 1.22, 1.17, 1.12, 1.07, 1.02, 0.97, 0.92, 0.87, 0.82, 0.77, 0.72, 0.67, 0.62, 0.57, 0.52,
          0.47, 0.42, 0.37, 0.32, 0.27, 0.22, 0.17, 0.12, 0.07]


def besseldbinverse(y):
    for t, x in zip(BINV_T, BINV_X):
        if y > t:
            return x
    return 0.0


def errnull(y):
    """BscanFFTpeak.cpp:397-415."""
    return 2.405 - besseldbinverse(y)


def to_nm(x, lambda0):
    """x * lambda0 * 1e9 / (4 * pi) in the reference's order (lambda0 a float, BscanFFTpeak.cpp:1151)."""
    return x * float(np.float32(lambda0)) * 1e9 / (4 * PI)


def picture(db, layout):
    """(n, ascans, depths) row-major or (n, depths, ascans) transposed -> (n, depths, ascans)."""
    a = np.asarray(db, np.float32)
    if a.ndim == 2:
        a = a[None]
    return a if layout == LAYOUT_TRANSPOSED else np.transpose(a, (0, 2, 1))


def min_max_ascan(pics, ascanat):
    """printMinMaxAscan, BscanFFT.cpp:146-171: rows 0-3 of a copy of A-scan ascanat <- row 4, then minMaxLoc."""
    col = pics[:, :, ascanat].copy()
    col[:, 0:4] = col[:, 4:5]
    return col.min(axis=1), col.max(axis=1)


def avg_roi(pics, ascanat, vertpos, width):
    """printAvgROI, BscanFFT.cpp:99-144: mean of bscandb(Rect(ascanat, vertpos, width, 3)), in double; None where the
    strict guard ascanat + width < cols (107) refuses."""
    if not ascanat + width < pics.shape[2]:
        return None
    return pics[:, vertpos:vertpos + 3, ascanat:ascanat + width].astype(np.float64).mean(axis=(1, 2))


class PeakHold:
    """printPeakHoldAscan's four hold slots (BscanFFTpeak.cpp:466-739) with onMouse's reset (175-179) and the ! @ # $ keys."""

    def __init__(self):
        self.roi = None
        self.cols = [None] * 4
        self.scalar = [0.0] * 4     # max1val .. max4val start at 0
        self.count = [0] * 4

    def set_roi(self, x, y, w, h, ascanat):
        self.roi = (x, y, w, h, ascanat)
        self.cols = [np.zeros(w, np.float64) for _ in range(4)]   # Mat::zeros(Size(ROIw, 1), CV_64F); scalars stay

    def clear(self, slot):
        if self.roi is not None:
            self.cols[slot - 1] = np.zeros(self.roi[2], np.float64)
        self.scalar[slot - 1] = 0.0
        self.count[slot - 1] = 0

    def fold(self, slot, pics):
        x, y, w, h, ascanat = self.roi
        for p in pics:
            maxval = float(p[y:y + h, ascanat].max())                          # minMaxLoc(ascan.rowRange(...)), 502-503
            if maxval > self.scalar[slot - 1]:
                self.scalar[slot - 1] = maxval
            maxarray = p[y:y + h, x:x + w].max(axis=0).astype(np.float64)      # reduce(bsdisp, .., 0, MAX), 505-507
            self.cols[slot - 1] = np.maximum(maxarray, self.cols[slot - 1])    # max(maxarray, max1vals), 523
            self.count[slot - 1] += 1

    def vibration(self, mode, lambda0):
        m1, m2, m3, m4 = self.scalar
        c1, _, c3, c4 = self.cols
        if mode == 3:                                                          # 597-644
            disp = to_nm(besseldbinverse(m1 - m3), lambda0)
            err = to_nm(errnull(m1 - m2), lambda0)
            prof = np.array([to_nm(besseldbinverse(d), lambda0) for d in c1 - c3])
        else:                                                                  # 681-731
            disp = to_nm(besseldbinverse(m1 - m4), lambda0)
            err = float("nan")                                                 # the reference prints an unset local
            p3 = np.array([to_nm(besseldbinverse(d), lambda0) for d in c1 - c3])
            p4 = np.array([to_nm(besseldbinverse(d), lambda0) for d in c1 - c4])
            prof = p3 - p4
        return prof, disp, err
