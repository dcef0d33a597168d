"""The specification of spinjnt's output binning (include/fdoct_bscanbin.h; BscanFFTspinjnt.cpp:1849-1874, 1894-1903) in numpy,
step by step as the header writes it, on pictures: arrays (depths, ascans), x along A-scans (axis 1), y along depths (axis 0).

Two modes:
  "truth"      everything in double.
  "reference"  double data with float32 taps built in float32 arithmetic and a float32 1 / area: what OpenCV's resize is
               believed to do on CV_64F images (nothing in this project can pin it).
Every sum runs in the written order; numpy only carries it over all cells / outputs at once."""
import numpy as np

A = -0.75
EPS_MAIN, EPS_SIM = float(np.float32(1e-5)), float(np.float32(1e-6))
MAX_FACTOR, MAX_UP = 16, 64


def out_size(depths, ascans, binx, biny, upx, upy):
    return depths // biny * upy, ascans // binx * upx


def taps(up, mode="truth"):
    """(taps float64 (up, 4), first source offset int (up,)): phase p of output d = k up + p reads cells k + off[p] .. + 3."""
    ft = np.float64 if mode == "truth" else np.float32
    a = ft(A)
    one, half = ft(1), ft(0.5)
    scale = one / ft(up)
    c = np.zeros((up, 4), np.float64)
    off = np.zeros(up, np.int64)
    for p in range(up):
        f = ft(ft(p) + half) * scale - half
        s = np.floor(f)
        t = ft(f - s)
        t1, u = ft(t + one), ft(one - t)
        c0 = ((a * t1 - ft(5) * a) * t1 + ft(8) * a) * t1 - ft(4) * a
        c1 = ((a + ft(2)) * t - (a + ft(3))) * t * t + one
        c2 = ((a + ft(2)) * u - (a + ft(3))) * u * u + one
        c3 = one - c0 - c1 - c2
        assert all(type(v) is ft for v in (c0, c1, c2, c3))
        c[p] = [c0, c1, c2, c3]
        off[p] = int(s) - 1
    return c, off


def lockin_input(pic, jscan):
    """1849-1852: max(bscan - jscan, 0) + 0.001, in double."""
    return np.maximum(pic.astype(np.float64) - jscan.astype(np.float64), 0.0) + 0.001


def area(v, binx, biny, multiplyfactor, mode="truth"):
    """INTER_AREA at integer factors times multiplyfactor: block sums, rows outermost, left to right within a row."""
    D, H = v.shape
    assert D % biny == 0 and H % binx == 0
    v = v.astype(np.float64)
    acc = np.zeros((D // biny, H // binx), np.float64)
    for dy in range(biny):
        for dx in range(binx):
            acc = acc + v[dy::biny, dx::binx]
    inv = 1.0 / (binx * biny) if mode == "truth" else float(np.float32(1) / np.float32(binx * biny))
    return acc * inv * float(multiplyfactor)


def _cubic_axis1(b, up, mode):
    n = b.shape[1]
    c, off = taps(up, mode)
    d = np.arange(n * up)
    k, p = d // up, d % up
    idx = [np.clip(k + off[p] + i, 0, n - 1) for i in range(4)]
    w = [c[p, i][None, :] for i in range(4)]
    return ((w[0] * b[:, idx[0]] + w[1] * b[:, idx[1]]) + w[2] * b[:, idx[2]]) + w[3] * b[:, idx[3]]


def cubic(b, upx, upy, mode="truth"):
    """INTER_CUBIC: along A-scans first, then along depths; each four-term sum left to right (top to bottom)."""
    h = _cubic_axis1(b, upx, mode)
    return np.ascontiguousarray(_cubic_axis1(np.ascontiguousarray(h.T), upy, mode).T)


def to_db(value, eps, mask):
    db = 20.0 * np.log(np.maximum(value, eps)) / 2.303
    if mask and db.shape[0] > 4:
        db[0] = db[4]
        db[1] = db[4]
    return db


def bscan_bin(pic, binx, biny, upx=None, upy=None, multiplyfactor=None, jscan=None, eps=EPS_MAIN, dc_mask=True, mode="truth"):
    """One picture (depths, ascans) -> (linear float64, dB float64) pictures of out_size()."""
    upx, upy = binx if upx is None else upx, biny if upy is None else upy
    mf = binx * biny if multiplyfactor is None else multiplyfactor
    v = pic.astype(np.float64) if jscan is None else lockin_input(pic, jscan)
    lin = cubic(area(v, binx, biny, mf, mode), upx, upy, mode)
    return lin, to_db(lin, eps, dc_mask and jscan is None)


# ---- an independent formulation: the same stage as dense matrices, U_y (A_y X A_x^T) U_x^T ------------------------------------
def area_matrix(n, bin_):
    m = np.zeros((n // bin_, n))
    for i in range(n // bin_):
        m[i, i * bin_:(i + 1) * bin_] = 1.0 / bin_
    return m


def cubic_matrix(n, up):
    """(n up, n): row d holds the four taps of output d, clamped indices accumulated."""
    m = np.zeros((n * up, n))
    for d in range(n * up):
        f = (d + 0.5) / up - 0.5
        s = int(np.floor(f))
        t = f - s
        w = [((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) ** 2 + 1]
        w.append(1 - sum(w))
        for i in range(4):
            m[d, min(max(s - 1 + i, 0), n - 1)] += w[i]
    return m


def dense(v, binx, biny, upx, upy, multiplyfactor):
    D, H = v.shape
    b = area_matrix(D, biny) @ v.astype(np.float64) @ area_matrix(H, binx).T * multiplyfactor
    return cubic_matrix(D // biny, upy) @ b @ cubic_matrix(H // binx, upx).T


# ---- the project's parity rule ------------------------------------------------------------------------------------------
def tolerance(truth):
    """1e-4 |truth| + 1e-6 max over the output A-scan (a column of the picture) of |truth|."""
    return 1e-4 * np.abs(truth) + 1e-6 * np.abs(truth).max(axis=-2, keepdims=True)


def parity(got_lin, got_db, pic, binx, biny, upx=None, upy=None, multiplyfactor=None, jscan=None, eps=EPS_MAIN, dc_mask=True,
           what=""):
    """Holds results (pictures; either may be None) to the truth-mode model on every element:
      linear  |got - truth| / tol <= max(0.5, |reference-mode - truth| / tol)
      dB      |got_db - truth_db| <= 8.686 tol / max(truth - tol, eps) + 2e-4 (rows under the DC mask: row 4's truth and tol)
    and truth <= 0 gives exactly dB(eps).  Returns (worst linear ratio, worst dB ratio, share of truth <= 0)."""
    kw = dict(upx=upx, upy=upy, multiplyfactor=multiplyfactor, jscan=jscan, eps=eps, dc_mask=dc_mask)
    truth, truth_db = bscan_bin(pic, binx, biny, mode="truth", **kw)
    ref, _ = bscan_bin(pic, binx, biny, mode="reference", **kw)
    tol = tolerance(truth)
    worst_lin = worst_db = 0.0
    if got_lin is not None:
        assert got_lin.shape == truth.shape, (what, got_lin.shape, truth.shape)
        err = np.abs(got_lin.astype(np.float64) - truth)
        bound = np.maximum(0.5 * tol, np.abs(ref - truth))
        worst_lin = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.max() > 0 else 0.0
        print("%s linear: worst |gpu - truth| / bound %.4f (reference mode at %.3f tol)" % (
            what, worst_lin, float((np.abs(ref - truth) / np.maximum(tol, 1e-300)).max())))
        assert (err <= bound).all(), "%s linear: %d elements beyond the bound, worst %.3f" % (what, int((err > bound).sum()), worst_lin)
    if got_db is not None:
        assert got_db.shape == truth.shape, (what, got_db.shape, truth.shape)
        assert np.isfinite(got_db).all(), what + ": dB not finite"
        t, tl = truth.copy(), tol.copy()
        if dc_mask and jscan is None and t.shape[0] > 4:
            t[0] = t[1] = t[4]
            tl[0] = tl[1] = tl[4]
        bound = 8.686 * tl / np.maximum(t - tl, eps) + 2e-4
        err = np.abs(got_db.astype(np.float64) - truth_db)
        worst_db = float((err / bound).max())
        print("%s dB: worst |gpu - truth| / bound %.4f" % (what, worst_db))
        assert (err <= bound).all(), "%s dB: %d elements beyond the bound, worst %.3f" % (what, int((err > bound).sum()), worst_db)
        floor = np.float32(20.0 * np.log(eps) / 2.303)
        assert (got_db[t <= 0] == floor).all(), what + ": truth <= 0 must give dB(eps) exactly"
    return worst_lin, worst_db, float((truth <= 0).mean())
