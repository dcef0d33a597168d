"""The specification of the Doppler stage (include/fdoct_doppler.h) in numpy, and the rule the library is held to.

The quantity.  X[f][r][b]: nframes images of ascans x depths complex A-scans.
    pair images   T[p][r][b] = X2 conj(X1);  A-scans (axis 0): X1 = X[f][r], X2 = X[f][r + lag], one image per frame of
                  ascans - lag rows;  frames (axis 1): X1 = X[f][r], X2 = X[f + lag][r], nframes - lag images of ascans rows.
    bulk          B[p][r] = sum of T[p][r][b] over b in [first, first + count) (count 0: all depths); T' = T conj(B) / |B|, and
                  T' = T where |B| = 0.  Without it T' = T.
    window        R[p][r][b] = sum of T' over r' in [r - (wa - 1) // 2, r + wa // 2] and b' in [b - (wd - 1) // 2, b + wd // 2],
                  truncated to the pair image; cnt = the number of terms left.
    power         P = sum of (|X1|^2 + |X2|^2) / 2 over the same window.
    outputs       phase = scale atan2(Im R, Re R), 0 where min_power > 0 and P / cnt < min_power;  corr = R;  power = P / cnt.

model(..., truth=False) is the float composition: float32 products and sums, the box sum taken along depth and then across rows,
each in increasing index -- the order the kernel takes them in.  model(..., truth=True) is everything in double.  brute() is the
definition as a double loop, the check of both.

The tolerance, u = 2^-24.  S = sum of |X1| |X2| over the window, K = wa wd its full number of terms.

  correlation   A complex float product (two products and a sum per component) is within 2 u |X1| |X2| (1 + O(u)) of the exact
                one -- "a few u"; a sum of K terms in any order is within (K - 1) u sum|t| of the exact sum (Higham, Accuracy and
                Stability, 4.2: recursive summation).  So |R_gpu - R_truth| <= tol_R = (K + 4) u S.
  with bulk     B is such a sum over the bulk range: |B_f32 - B_truth| <= tol_B = (depths + 4) u sum_b |t|, the sum over the
                range.  The phasor conj(B) / |B| moves by at most |dB| / |B| for |dB| << |B| (a unit vector's change under a
                perturbation of its argument's numerator, first order; the cases keep |B| >= 16 tol_B, so the second-order term
                is below 1/16 of it and is covered by the 4 u that follows), the normalisation -- a hypot and two divisions --
                and the product T conj(phasor) add the same "few u" as a complex product: 4 u.  Every term of row r' is thus
                off by |t| (tol_B[r'] / |B[r']| + 4 u) on top of its own rounding, and
                tol_R = (K + 4) u S + sum over the window of |t| (tol_B[r'] / |B[r']| + 4 u).  Rows of zeros (T = 0, B = 0 exactly: the
                cases' zero rows) add nothing.
  power         |P_gpu - P_truth| <= (K + 4) u P, so out_power is held to tol_P = (K + 4) u P / cnt.
  phase         held to the kernel's own written correlation, which is itself held to the truth:
                |wrap(phase_gpu / scale - atan2(R_gpu in double))| <= PHASE_TOL = 4 ATAN2F_HOST + 2 pi u.  ATAN2F_HOST is the worst
                |float32 arctan2 - float64 arctan2| of the float composition's R over every case of tests/doppler_cases.py,
                measured on the CPU: 2.67e-07 rad (the one-pair-row case; the others 3e-08 .. 2.2e-07), recorded below as
                2.7e-07; tests/test_doppler_cases.py prints each case's figure and asserts it does not exceed the record.  The
                device's libm is granted more ulps than the host's: 4 x that, 1.08e-06.  2 pi u is the final multiply by scale,
                at most half an ulp of an angle below 2 pi.  PHASE_TOL = 1.45e-06 rad; the check uses the constant, never a
                value computed from the GPU result.

The adjudication is the project's own: |gpu - truth| / tol <= max(helpers.TRUTH_LIMIT, the float composition's own ratio), every
figure printed first and appended to helpers.TRUTH_LOG.

Exemptions, each capped at 1 % of a case's bins (tests/test_doppler_cases.py asserts that from this model alone):
    bins with |R_truth| < 16 tol_R are exempt from the phase check;
    bins with |P_truth / cnt - min_power| <= tol_P are exempt from the mask check (on which side of min_power they fall)."""
import os

import numpy as np

import helpers

U = 2.0 ** -24
ATAN2F_HOST = 2.7e-07                         # rad; measured 2.67e-07 (see above)
PHASE_TOL = 4 * ATAN2F_HOST + 2 * np.pi * U   # rad
ASCANS, FRAMES = 0, 1
RATIOS = []   # (what, corr gpu/truth, corr f32/truth, power gpu/truth, power f32/truth, worst phase error / PHASE_TOL), one per check()


def pair_shape(axis, lag, nframes, ascans):
    return (nframes - lag, ascans) if axis == FRAMES else (nframes, ascans - lag)


def pairs(X, axis, lag):
    """(X1, X2), each (pair_images, pair_rows, depths)."""
    X = np.asarray(X)
    assert X.ndim == 3 and lag >= 1
    if axis == FRAMES:
        assert X.shape[0] > lag
        return X[:-lag], X[lag:]
    assert X.shape[1] > lag
    return X[:, :-lag], X[:, lag:]


def _shift_add(acc, t, off, axis):
    """acc[i] += t[i + off] along `axis` where i + off lies in the image."""
    n = t.shape[axis]
    lo, hi = max(0, -off), min(n, n - off)
    if lo >= hi:
        return
    dst = [slice(None)] * t.ndim
    src = [slice(None)] * t.ndim
    dst[axis], src[axis] = slice(lo, hi), slice(lo + off, hi + off)
    acc[tuple(dst)] += t[tuple(src)]


def box(t, wa, wd):
    """The window's sum of t (pair_images, pair_rows, depths) in t's own type: along depth first, then across rows, each in
    increasing index; truncated to the image."""
    d = np.zeros_like(t)
    for j in range(wd):
        _shift_add(d, t, j - (wd - 1) // 2, 2)
    r = np.zeros_like(t)
    for j in range(wa):
        _shift_add(r, d, j - (wa - 1) // 2, 1)
    return r


def count(pair_rows, depths, wa, wd):
    """cnt (pair_rows, depths): the window's overlap with the pair image."""
    r, b = np.arange(pair_rows), np.arange(depths)
    nr = np.minimum(r + wa // 2, pair_rows - 1) - np.maximum(r - (wa - 1) // 2, 0) + 1
    nb = np.minimum(b + wd // 2, depths - 1) - np.maximum(b - (wd - 1) // 2, 0) + 1
    return nr[:, None] * nb[None, :]


def bulk_range(bulk, depths):
    """(first, count) of the bulk sum, or None: bulk is None / False, True (all depths) or (first, count), count 0 meaning the rest."""
    if bulk is None or bulk is False:
        return None
    first, cnt = (0, 0) if bulk is True else bulk
    return first, cnt if cnt else depths - first


def model(X, axis, lag, win=(1, 1), bulk=None, scale=1.0, min_power=0.0, truth=False):
    """dict(phase, corr, power, cnt [, B]): float32 / complex64, or float64 / complex128 with truth."""
    wa, wd = win
    X1, X2 = pairs(X, axis, lag)
    f = np.float64 if truth else np.float32
    a, b, c, d = X1.real.astype(f), X1.imag.astype(f), X2.real.astype(f), X2.imag.astype(f)
    re, im = c * a + d * b, d * a - c * b                       # X2 conj(X1)
    pw = (a * a + b * b) + (c * c + d * d)
    out = {}
    rng = bulk_range(bulk, X1.shape[2])
    if rng:
        first, cnt = rng
        if truth:
            Br, Bi = re[..., first:first + cnt].sum(-1), im[..., first:first + cnt].sum(-1)
        else:   # the kernel's order is a strided partial per thread and a tree; any order is within tol_B, this one is numpy's
            Br, Bi = re[..., first:first + cnt].sum(-1, dtype=f), im[..., first:first + cnt].sum(-1, dtype=f)
        m = np.hypot(Br, Bi).astype(f)
        ok = m > 0
        ur = np.where(ok, Br / np.where(ok, m, 1), 1).astype(f)[..., None]
        ui = np.where(ok, Bi / np.where(ok, m, 1), 0).astype(f)[..., None]
        re, im = re * ur + im * ui, im * ur - re * ui           # T conj(B / |B|)
        out["B"] = Br + 1j * Bi
    R_re, R_im, P = box(re, wa, wd), box(im, wa, wd), box(pw, wa, wd)
    cnt = count(X1.shape[1], X1.shape[2], wa, wd)
    power = (f(0.5) * P / cnt.astype(f)).astype(f)
    phase = (f(scale) * np.arctan2(R_im, R_re)).astype(f)
    if min_power > 0:
        phase = np.where(power < f(min_power), f(0), phase)
    out.update(phase=phase, corr=(R_re + 1j * R_im).astype(np.complex128 if truth else np.complex64), power=power, cnt=cnt)
    return out


def brute(X, axis, lag, win=(1, 1), bulk=None):
    """R, P / cnt and cnt by the definition, a double loop over the window in double."""
    wa, wd = win
    X1, X2 = (np.asarray(v, np.complex128) for v in pairs(X, axis, lag))
    T = X2 * np.conj(X1)
    rng = bulk_range(bulk, T.shape[2])
    if rng:
        B = T[..., rng[0]:rng[0] + rng[1]].sum(-1, keepdims=True)
        m = np.abs(B)
        T = T * np.where(m > 0, np.conj(B) / np.where(m > 0, m, 1), 1)
    pw = (np.abs(X1) ** 2 + np.abs(X2) ** 2) / 2
    PI, PR, D = T.shape
    R, P, cnt = np.zeros(T.shape, np.complex128), np.zeros(T.shape), np.zeros((PR, D), np.int64)
    for r in range(PR):
        for b in range(D):
            r0, r1 = max(r - (wa - 1) // 2, 0), min(r + wa // 2, PR - 1)
            b0, b1 = max(b - (wd - 1) // 2, 0), min(b + wd // 2, D - 1)
            R[:, r, b] = T[:, r0:r1 + 1, b0:b1 + 1].sum((1, 2))
            P[:, r, b] = pw[:, r0:r1 + 1, b0:b1 + 1].sum((1, 2))
            cnt[r, b] = (r1 - r0 + 1) * (b1 - b0 + 1)
    return R, P / cnt, cnt


def tolerances(X, axis, lag, win=(1, 1), bulk=None):
    """dict(tol_R, tol_P, S [, tol_B, B]) from the truth alone, per bin (tol_B and B per pair row)."""
    wa, wd = win
    K = wa * wd
    X1, X2 = (np.asarray(v, np.complex128) for v in pairs(X, axis, lag))
    t = np.abs(X1) * np.abs(X2)
    S = box(t, wa, wd)
    tol_R = (K + 4) * U * S
    out = {}
    rng = bulk_range(bulk, t.shape[2])
    if rng:
        first, cnt = rng
        B = (X2 * np.conj(X1))[..., first:first + cnt].sum(-1)
        tol_B = (t.shape[2] + 4) * U * t[..., first:first + cnt].sum(-1)
        live = tol_B > 0   # (a row of zeros has B = 0, tol_B = 0 and terms of 0: nothing to add)
        e = np.where(live, tol_B / np.where(live, np.abs(B), 1) + 4 * U, 0)
        tol_R = tol_R + box(t * e[..., None], wa, wd)
        out.update(tol_B=tol_B, B=B)
    P = box((np.abs(X1) ** 2 + np.abs(X2) ** 2) / 2, wa, wd)
    out.update(tol_R=tol_R, S=S, tol_P=(K + 4) * U * P / count(t.shape[1], t.shape[2], wa, wd))
    return out


def wrap(a):
    return (np.asarray(a, np.float64) + np.pi) % (2 * np.pi) - np.pi


def _ratio(got, ref, tol):
    """Worst |got - ref| / tol; a bin with tol = 0 (a window of zeros) must hold the reference itself."""
    err = np.abs(np.asarray(got, np.complex128) - ref)
    return float(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err == 0, 0, np.inf)).max())


def exemptions(X, axis, lag, win=(1, 1), bulk=None, min_power=0.0):
    """(phase-exempt bins, mask-exempt bins) as boolean arrays, from the truth alone."""
    tr = model(X, axis, lag, win, bulk, truth=True)
    tol = tolerances(X, axis, lag, win, bulk)
    ill = np.abs(tr["corr"]) < 16 * tol["tol_R"]
    edge = np.abs(tr["power"] - min_power) <= tol["tol_P"] if min_power > 0 else np.zeros(ill.shape, bool)
    return ill, edge


def check(gpu, X, axis, lag, what, win=(1, 1), bulk=None, scale=1.0, min_power=0.0):
    """gpu: dict(phase, corr, power) as the library wrote them.  Correlation and power against the truth by the adjudication,
    the phase against the written correlation, the mask exactly; every figure printed before anything is asserted."""
    phase, corr, power = (np.asarray(gpu[k]) for k in ("phase", "corr", "power"))
    assert phase.dtype == power.dtype == np.float32 and corr.dtype == np.complex64, what
    for v in (phase, power, corr.view(np.float32)):
        assert np.isfinite(v).all(), what + ": not finite (an output bin was not written)"
    ref = model(X, axis, lag, win, bulk, scale, min_power)
    tr = model(X, axis, lag, win, bulk, scale, min_power, truth=True)
    tol = tolerances(X, axis, lag, win, bulk)
    assert corr.shape == tr["corr"].shape == phase.shape == power.shape, (corr.shape, tr["corr"].shape)
    gR, oR = _ratio(corr, tr["corr"], tol["tol_R"]), _ratio(ref["corr"], tr["corr"], tol["tol_R"])
    gP, oP = _ratio(power, tr["power"], tol["tol_P"]), _ratio(ref["power"], tr["power"], tol["tol_P"])
    ill, edge = exemptions(X, axis, lag, win, bulk, min_power)
    if min_power > 0:
        below = (tr["power"] < min_power) & ~edge
        above = (tr["power"] >= min_power) & ~edge
    else:
        below, above = np.zeros(ill.shape, bool), np.ones(ill.shape, bool)
    own = np.arctan2(corr.imag.astype(np.float64), corr.real.astype(np.float64))
    perr = np.abs(wrap(phase.astype(np.float64) / scale - own))
    held = above & ~ill
    worst = float(perr[held].max()) if held.any() else 0.0
    unmasked = int(np.count_nonzero(phase[below]))
    print("%s: corr |gpu - truth| / tol = %.4f (f32 model %.4f), power %.4f (f32 model %.4f), phase error %.3g rad = %.3f of PHASE_TOL "
          "over %d bins (%d exempt), %d masked bins of which %d not 0" % (what, gR, oR, gP, oP, worst, worst / PHASE_TOL, int(held.sum()),
                                                                         int(ill.sum()), int(below.sum()), unmasked))
    RATIOS.append((what, gR, oR, gP, oP, worst / PHASE_TOL))
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    helpers.TRUTH_LOG.append((test, what + " (doppler corr)", gR, oR))
    helpers.TRUTH_LOG.append((test, what + " (doppler power)", gP, oP))
    assert gR <= max(helpers.TRUTH_LIMIT, oR), "%s: corr |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 model's own %.3g)" % (
        what, gR, helpers.TRUTH_LIMIT, oR)
    assert gP <= max(helpers.TRUTH_LIMIT, oP), "%s: power |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 model's own %.3g)" % (
        what, gP, helpers.TRUTH_LIMIT, oP)
    assert worst <= PHASE_TOL, "%s: the phase is %.3g rad off its own correlation's angle, beyond %.3g" % (what, worst, PHASE_TOL)
    assert unmasked == 0, "%s: %d bins below min_power are not 0" % (what, unmasked)
    if min_power > 0:   # an unmasked bin of a live field has an angle: all of them 0 would be a mask that covers everything
        assert not above.any() or np.count_nonzero(phase[above]) > 0, what + ": every bin above min_power is 0"
    return gR, oR, gP, oP, worst
