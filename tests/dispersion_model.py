"""The specification of the dispersion search (include/fdoct_dispersion.h) in numpy, and the rule the library is held to.

The quantity.  X[r][b]: rows complex A-scans of the full transform length n.
    spectrum     z[r][q] = (1/n) sum_b X[r][b] e^(-2 pi i b q / n)
    candidates   a2_i = a2_first + i a2_step, a3_j = a3_first + j a3_step, c = i a3_count + j, K = a2_count a3_count
    phase        phi_c(q) = a2 x^2 + a3 x^3, x = (q - n/2) / (n/2)                (synth.dispersion_phase's convention)
    A-scan       A_c[r][b] = sum_q z[r][q] e^(i phi_c(q)) e^(+2 pi i b q / n)     (the chain's unscaled inverse)
    sums         I = |A_c|^2;  S2[r][c] = sum I, S4[r][c] = sum I^2 over b in [depth_first, depth_first + depth_count),
                 depth_count = 0 meaning up to n // 2;  S2[c], S4[c] the sums over rows in increasing row order
    metric       S4[c] / S2[c]^2, 0 where S2[c] = 0
    winner       the lowest index of the largest finite metric, -1 if none is finite

model(..., truth=False) is the float composition: scipy.fft on complex64 both ways, the 1/n as a float multiply, the phasor as the
complex64 product of e^(i a2 x^2) and e^(i a3 x^3), each evaluated in double and rounded to float, I and I^2 in float32, every sum in
double.  model(..., truth=True) is everything in double.  brute() is the definition as a double loop over (row, candidate) with
the transforms as matrix products, the check of both.

The tolerance, u = 2^-24.
    A float FFT of n points has a norm-wise error of at most about 7 u log2 n (Higham, Accuracy and Stability of Numerical
    Algorithms, Theorem 24.2: ||y_f32 - y|| / ||y|| <= log2 n  mu / (1 - log2 n  mu) with mu a few u for radix-2 butterflies with
    computed twiddles).  The stage runs two of them -- 14 u log2 n, taken as 16 u log2 n -- and between them the phasor's two
    roundings (u each), its complex product and the product with z (a few u each) and the multiply by 1/n (u): 8 u.  So
        g = (16 log2 n + 8) u                      the stage's norm-wise relative error
        eps_r = g ||A_r||_2                        over the FULL length (the error of one bin is bounded by the row's norm, not by
                                                   the bin), the same for every candidate up to rounding: Parseval, |phasor| = 1
    and for sums over any range of bins, by Cauchy-Schwarz on sum (|A + e|^2 - |A|^2) = sum (2 Re(conj(A) e) + |e|^2):
        tol_S2[r][c] = 2 sqrt(S2[r][c]) eps_r + eps_r^2
        tol_S4[r][c] = 2 max_b(I) tol_S2[r][c] + 2 u S4[r][c]
    (I^2 - I'^2 = (I + I')(I - I') with I + I' <= 2 max I to first order; 2 u S4: the float I and the float square round once
    each).  The sums in double add nothing that shows at this scale.  Over rows the tolerances add.  A row of zeros has tolerance 0
    and must come back as exact zeros.

The adjudication is the project's own: |gpu - truth| / tol <= max(helpers.TRUTH_LIMIT, the float composition's own ratio), every
figure printed first and appended to helpers.TRUTH_LOG.  The float composition sits at <= 0.011 of the bound on the cases of
tests/dispersion_cases.py (tests/test_dispersion_cases.py prints each case's figure).

Measured on an MI355X (profiles/dispersion_ratios.txt): the library's worst |gpu - truth| / tol over those cases is 0.0184 for S2
(128 x 4, planted (12, -4)) and 0.0112 for S4 (the same field with a zero row), where the float composition's worst are 0.0105 and
0.0083: about twice scipy's, below 0.1, and 1/27 of the limit of 0.5.

The winner.  The library's winner must be the truth's.  That is a fair demand only where the truth's best metric stands clear of
its second best by more than the tolerance can move either: tests/test_dispersion_cases.py asserts, from this model alone, that
every case's margin (best / second best) is at least 1 + 64 x the case's largest relative tolerance (tol / value over S2[c] and
S4[c] of every candidate)."""
import os

import numpy as np

import helpers

U = 2.0 ** -24
GPU_WORST_S2 = 0.0184   # measured (profiles/dispersion_ratios.txt); a record, not a bound: the bound is check()'s
GPU_WORST_S4 = 0.0112
RATIOS = []   # (what, S2 gpu/tol, S2 f32/tol, S4 gpu/tol, S4 f32/tol), one per check()


def axis_values(first, step, count):
    """first + i step, as the library evaluates it (double)."""
    return np.float64(first) + np.arange(int(count), dtype=np.float64) * np.float64(step)


def depth_range(n, depth):
    first, count = depth
    return int(first), int(first) + (int(count) if count else n // 2 - int(first))


def x_of(n):
    return (np.arange(n, dtype=np.float64) - n / 2) / (n / 2)


def phase_table(n, a2, a3):
    """(n, 2) float32 (cos, sin) of phi = a2 x^2 + a3 x^3 in double, rounded: what fdoct_dispersion_phase_table writes."""
    x = x_of(n)
    phi = a2 * (x * x) + a3 * (x * x * x)
    return np.stack([np.cos(phi), np.sin(phi)], axis=1).astype(np.float32)


def phasors(n, a2, a3, truth):
    """(K, n) phasors of the grid: complex128, or the complex64 product of the two rounded tables."""
    x = x_of(n)
    p2 = np.exp(1j * axis_values(*a2)[:, None] * (x * x)[None, :])
    p3 = np.exp(1j * axis_values(*a3)[:, None] * (x * x * x)[None, :])
    if not truth:
        p2, p3 = p2.astype(np.complex64), p3.astype(np.complex64)
    return (p2[:, None, :] * p3[None, :, :]).reshape(-1, n)


def ascans(X, a2, a3, truth):
    """A[r][c][b], (rows, K, n)."""
    X = np.asarray(X)
    n = X.shape[-1]
    X = X.reshape(-1, n)
    ph = phasors(n, a2, a3, truth)
    if truth:
        z = np.fft.fft(X.astype(np.complex128), axis=-1) / n
        return np.fft.ifft(z[:, None, :] * ph[None, :, :], axis=-1) * n
    import scipy.fft
    z = scipy.fft.fft(X.astype(np.complex64), axis=-1) * np.float32(1.0 / n)
    assert z.dtype == np.complex64
    w = (z[:, None, :] * ph[None, :, :]).astype(np.complex64)
    A = scipy.fft.ifft(w, axis=-1, norm="forward")
    assert A.dtype == np.complex64
    return A


def metrics(sums):
    s2, s4 = sums[:, 0], sums[:, 1]
    with np.errstate(all="ignore"):
        return np.where(s2 == 0, 0.0, s4 / (s2 * s2))


def winner(metric):
    ok = np.isfinite(metric)
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, metric, -np.inf)))   # argmax: the first of equals


def model(X, a2, a3, depth=(0, 0), truth=False):
    """dict: row_sums (rows, K, 2), sums (K, 2), metric (K,), index, and -- for the tolerance -- norm (rows, K) = ||A_r||_2 over the
    full length and peak (rows, K) = max I over the depth range."""
    A = ascans(X, a2, a3, truth)
    n = A.shape[-1]
    b0, b1 = depth_range(n, depth)
    if truth:
        I = A.real * A.real + A.imag * A.imag
        I2 = I * I
    else:
        re, im = A.real.astype(np.float32), A.imag.astype(np.float32)
        I = re * re + im * im
        I2 = I * I
        assert I2.dtype == np.float32
    Id, I2d = I.astype(np.float64), I2.astype(np.float64)
    row_sums = np.stack([Id[..., b0:b1].sum(-1), I2d[..., b0:b1].sum(-1)], axis=-1)
    sums = np.zeros(row_sums.shape[1:], np.float64)
    for r in range(row_sums.shape[0]):   # in increasing row order
        sums += row_sums[r]
    m = metrics(sums)
    return dict(row_sums=row_sums, sums=sums, metric=m, index=winner(m), norm=np.sqrt(Id.sum(-1)), peak=Id[..., b0:b1].max(-1))


def brute(X, a2, a3, depth=(0, 0)):
    """The definition as a double loop over (row, candidate), in double, the transforms as matrix products: (row_sums, sums)."""
    X = np.asarray(X).astype(np.complex128)
    n = X.shape[-1]
    X = X.reshape(-1, n)
    b0, b1 = depth_range(n, depth)
    q = np.arange(n)
    Wf = np.exp(-2j * np.pi * np.outer(q, q) / n)   # [q][b]
    Wi = np.exp(+2j * np.pi * np.outer(q, q) / n)   # [b][q]
    x = x_of(n)
    v2, v3 = axis_values(*a2), axis_values(*a3)
    out = np.zeros((X.shape[0], len(v2) * len(v3), 2))
    for r in range(X.shape[0]):
        z = Wf @ X[r] / n
        for c in range(out.shape[1]):
            i, j = divmod(c, len(v3))
            A = Wi @ (z * np.exp(1j * (v2[i] * x ** 2 + v3[j] * x ** 3)))
            I = np.abs(A[b0:b1]) ** 2
            out[r, c] = I.sum(), (I * I).sum()
    return out, out.sum(0)


def tolerances(t, n):
    """(tol_row_sums (rows, K, 2), tol_sums (K, 2)) from the truth model `t` of rows of n points."""
    g = (16.0 * np.log2(n) + 8.0) * U
    eps = g * t["norm"]
    s2, s4 = t["row_sums"][..., 0], t["row_sums"][..., 1]
    tol2 = 2.0 * np.sqrt(s2) * eps + eps * eps
    tol4 = 2.0 * t["peak"] * tol2 + 2.0 * U * s4
    tol_rows = np.stack([tol2, tol4], axis=-1)
    return tol_rows, tol_rows.sum(0)


def margin(t):
    """best / second-best metric of the truth model (inf with one candidate)."""
    m = np.sort(t["metric"][np.isfinite(t["metric"])])
    return float("inf") if m.size < 2 or m[-2] == 0 else float(m[-1] / m[-2])


def largest_relative_tolerance(t, n):
    _, tol = tolerances(t, n)
    with np.errstate(all="ignore"):
        rel = np.where(t["sums"] > 0, tol / t["sums"], 0.0)
    return float(rel.max())


def _ratio(got, want, tol):
    """max |got - want| / tol; where tol is 0 the values must be equal (ratio 0) -- inf otherwise.  NaN in got: inf."""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(all="ignore"):
        r = np.where(tol > 0, d / tol, np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def ratios(got_row_sums, got_sums, t, n):
    """(S2 ratio, S4 ratio) of a result against the truth model t: the worst over row_sums and sums."""
    tol_rows, tol_sums = tolerances(t, n)
    out = []
    for k in (0, 1):
        r = []
        if got_row_sums is not None:
            r.append(_ratio(got_row_sums[..., k], t["row_sums"][..., k], tol_rows[..., k]))
        if got_sums is not None:
            r.append(_ratio(got_sums[..., k], t["sums"][..., k], tol_sums[..., k]))
        out.append(max(r))
    return tuple(out)


def ulp_apart(a, b):
    """Largest distance of two float32 arrays in units of the larger value's spacing."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp).max())


def check(out, X, a2, a3, depth, what, t=None, f=None):
    """Holds a library result (dict with any of sums, row_sums, best, cos_sin) to the model: the sums by the adjudication, the
    winner equal to the truth's, the table within one float ulp of the winner's phase table.  t, f: the truth and float models where
    the caller has them already.  Returns the ratios."""
    n = np.asarray(X).shape[-1]
    t = t if t is not None else model(X, a2, a3, depth, truth=True)
    f = f if f is not None else model(X, a2, a3, depth, truth=False)
    g2, g4 = ratios(out.get("row_sums"), out.get("sums"), t, n)
    o2, o4 = ratios(f["row_sums"], f["sums"], t, n)
    print("%s: S2 |gpu - truth| / tol = %.4g (f32 composition %.4g), S4 %.4g (f32 composition %.4g)" % (what, g2, o2, g4, o4))
    RATIOS.append((what, g2, o2, g4, o4))
    tid = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    helpers.TRUTH_LOG.append((tid, what + " S2", g2, o2))
    helpers.TRUTH_LOG.append((tid, what + " S4", g4, o4))
    assert g2 <= max(helpers.TRUTH_LIMIT, o2), "%s: S2 |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 composition's own %.3g)" % (what, g2, helpers.TRUTH_LIMIT, o2)
    assert g4 <= max(helpers.TRUTH_LIMIT, o4), "%s: S4 |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 composition's own %.3g)" % (what, g4, helpers.TRUTH_LIMIT, o4)
    if "best" in out:
        b = out["best"]
        assert b["index"] == t["index"], "%s: the winner is %d, the truth's is %d" % (what, b["index"], t["index"])
        i2, i3 = divmod(t["index"], int(a3[2]))
        assert (b["i2"], b["i3"]) == (i2, i3)
        assert b["a2"] == axis_values(*a2)[i2] and b["a3"] == axis_values(*a3)[i3]
        want = metrics(np.asarray(out["sums"]))[t["index"]] if "sums" in out else None
        if want is not None:
            assert b["metric"] == want, "%s: the winner's metric is not S4 / S2^2 of the sums returned" % what
    if "cos_sin" in out:
        i2, i3 = divmod(t["index"], int(a3[2]))
        table = phase_table(n, axis_values(*a2)[i2], axis_values(*a3)[i3])
        d = ulp_apart(out["cos_sin"], table)
        print("%s: winner's table within %.3g float ulp of the phase table" % (what, d))
        assert d <= 1.0, "%s: out_cos_sin is %.3g ulp from the winner's phase table" % (what, d)
    return g2, o2, g4, o4
