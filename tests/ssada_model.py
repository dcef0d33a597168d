"""The specification of split-spectrum amplitude decorrelation (include/fdoct_ssada.h) in numpy, and the rule the library is held to.

The quantity.  X[g][n][r][b]: groups x repeats images of ascans A-scans of the full transform length N; M = bands, R = repeats.
    spectrum     z[q] = (1/N) sum_b X[b] e^(-2 pi i b q / N)                      per A-scan
    bands        support [k_first, k_first + k_count), k_count = 0 meaning up to N; s = k_count / M; c_m = k_first + (m + 1/2) s - 1/2;
                 G_m(q) = exp(-1/2 ((q - c_m) / sigma)^2) inside the support, exactly 0 outside; double, rounded to float
    band A-scan  A_m[b] = sum_q z[q] G_m(q) e^(+2 pi i b q / N)                   (the chain's unscaled inverse), kept for b in
                 [depth_first, depth_first + depth_count), depth_count = 0 meaning up to N // 2
    per band     d[g][m], p[g][m] = angio_model's decorr and power of the R band images of position g, window win, no mask
    means        decorr = (sum_m d) / M, power = (sum_m p) / M: float32 sums in increasing m, one division by float32(M);
                 decorr = 0 where min_power > 0 and power < min_power

model(..., truth=False) is the float composition: np.fft on complex64-rounded steps (the spectrum times float32(1/N) rounded to
complex64, the product with the float table rounded, the inverse rounded), then angio_model's float composition per band and the
float32 means.  model(..., truth=True) is everything in double from the definitions (the table in double, not rounded).  brute()
is the band A-scans by a direct O(N^2) DFT, for the smallest cases.

The tolerance of the band A-scans, from the truth alone, u = 2^-24:
        g = (16 log2 N + 8) u
tests/dispersion_model.py's stage error -- two float transforms (7 u log2 N each by Higham's Theorem 24.2, taken as 8) and between
them one product: here the table's rounding (u), the product with z (u a component) and the multiply by 1/N (u), well inside the
8 u the dispersion stage's phasor product needed.  Per A-scan and band
        || A_gpu - A_truth ||_2 <= g || A_truth ||_2     the left norm over the depths kept, the right one over all N bins
        | A_gpu - A_truth |     <= g || A_truth ||_2     per bin: a bin's error cannot exceed the row's
A row of zeros has tolerance 0 and must come back as exact zeros.  The adjudication is the project's own: |gpu - truth| / tol <=
max(helpers.TRUTH_LIMIT, the float composition's own ratio), no bin exempt, every figure printed first and appended to
helpers.TRUTH_LOG.

The decorrelation outputs are not held to a tolerance of their own: out_band_decorr and the per-band power are fdoct_angio's
kernel on out_bands, held bit for bit to angiography.angio_device on the same pairs (whose own tolerance tests/angio_model.py
carries), and out_decorr / out_power are the float32 band means of those, held bit for bit to band_mean() below."""
import os

import numpy as np

import angio_model as am
import helpers

U = 2.0 ** -24
RATIOS = []   # (what, row gpu/tol, row f32/tol, bin gpu/tol, bin f32/tol), one per check_bands()


def resolve(N, bands, sigma=None, support=(0, 0), depth=(0, 0)):
    """(k_first, k_count, sigma, depth_first, depth_count), resolved as the library resolves them."""
    k0, kc = int(support[0]), int(support[1])
    kc = kc if kc else N - k0
    d0, dc = int(depth[0]), int(depth[1])
    dc = dc if dc else N // 2 - d0
    sg = 0.5 * kc / bands if sigma is None else float(sigma)
    return k0, kc, sg, d0, dc


def band_table(N, bands, sigma=None, support=(0, 0), truth=False):
    """G (bands, N): float32 (double rounded to float), or with truth the doubles themselves."""
    k0, kc, sg, _, _ = resolve(N, bands, sigma, support)
    q = np.arange(N, dtype=np.float64)
    s = np.float64(kc) / np.float64(bands)
    G = np.zeros((bands, N), np.float64)
    inside = (q >= k0) & (q < k0 + kc)
    for m in range(bands):
        c = np.float64(k0) + (np.float64(m) + 0.5) * s - 0.5
        t = (q - c) / np.float64(sg)
        G[m] = np.where(inside, np.exp(-0.5 * (t * t)), 0.0)
    return G if truth else G.astype(np.float32)


def band_ascans(X, bands, sigma=None, support=(0, 0), truth=False):
    """A[f][m][r][b] over the FULL length: (nframes, bands, ascans, N), complex128 or complex64."""
    X = np.asarray(X)
    N = X.shape[-1]
    G = band_table(N, bands, sigma, support, truth)
    if truth:
        z = np.fft.fft(X.astype(np.complex128), axis=-1) / N
        return np.fft.ifft(z[:, None, :, :] * G[None, :, None, :], axis=-1) * N
    z = (np.fft.fft(X.astype(np.complex64), axis=-1).astype(np.complex64) * np.float32(1.0 / N)).astype(np.complex64)
    w = (z[:, None, :, :] * G[None, :, None, :]).astype(np.complex64)
    return (np.fft.ifft(w, axis=-1) * N).astype(np.complex64)


def brute(X, bands, sigma=None, support=(0, 0)):
    """The band A-scans over the full length from the definition, in double, the transforms as matrix products."""
    X = np.asarray(X).astype(np.complex128)
    N = X.shape[-1]
    q = np.arange(N)
    Wf = np.exp(-2j * np.pi * np.outer(q, q) / N)
    Wi = np.exp(+2j * np.pi * np.outer(q, q) / N)
    G = band_table(N, bands, sigma, support, truth=True)
    z = X @ Wf.T / N
    return np.stack([(z * G[m]) @ Wi.T for m in range(bands)], axis=1)


def layout(A, repeats, d0, dc):
    """out_bands' layout (groups, bands, repeats, ascans, Dc) from A (nframes, bands, ascans, N)."""
    T, M, H, N = A.shape
    return np.ascontiguousarray(A.reshape(T // repeats, repeats, M, H, N).transpose(0, 2, 1, 3, 4)[..., d0:d0 + dc])


def band_mean(band_values, min_power=0.0, band_power=None):
    """The float32 mean over axis 1 in increasing m, one division by float32(M); with band_power the mask is applied too: returns
    the mean, or (decorr, power)."""
    v = np.asarray(band_values, np.float32)
    M = v.shape[1]

    def mean(a):
        s = np.zeros(a.shape[:1] + a.shape[2:], np.float32)
        for m in range(M):
            s = (s + a[:, m]).astype(np.float32)
        return (s / np.float32(M)).astype(np.float32)

    if band_power is None:
        return mean(v)
    power = mean(np.asarray(band_power, np.float32))
    decorr = mean(v)
    if min_power > 0:
        decorr = np.where(power < np.float32(min_power), np.float32(0), decorr)
    return decorr, power


def model(X, repeats, bands, sigma=None, support=(0, 0), depth=(0, 0), win=(1, 1), min_power=0.0, truth=False):
    """dict: bands (groups, M, R, ascans, Dc), band_decorr and band_power (groups, M, ascans, Dc), decorr and power (groups, ascans,
    Dc), and -- for the tolerance -- norm (groups, M, R, ascans) = ||A||_2 over the full length."""
    X = np.asarray(X)
    N = X.shape[-1]
    _, _, _, d0, dc = resolve(N, bands, sigma, support, depth)
    A = band_ascans(X, bands, sigma, support, truth)
    T, M, H, _ = A.shape
    G = T // repeats
    norm = np.sqrt((np.abs(A.astype(np.complex128)) ** 2).sum(-1)).reshape(G, repeats, M, H).transpose(0, 2, 1, 3)
    B = layout(A, repeats, d0, dc)
    bd = np.empty((G, M, H, dc), np.float64 if truth else np.float32)
    bp = np.empty_like(bd)
    for g in range(G):
        for m in range(M):
            o = am.model(B[g, m], repeats, win=win, truth=truth)
            bd[g, m], bp[g, m] = o["decorr"][0], o["power"][0]
    if truth:
        power = bp.mean(1)
        decorr = bd.mean(1)
        if min_power > 0:
            decorr = np.where(power < min_power, 0.0, decorr)
    else:
        decorr, power = band_mean(bd, min_power, bp)
    return dict(bands=B, band_decorr=bd, band_power=bp, decorr=decorr, power=power, norm=norm)


def stage_error(N):
    return (16.0 * np.log2(N) + 8.0) * U


def band_ratios(got, t, N):
    """(row ratio, bin ratio) of band A-scans `got` (groups, M, R, ascans, Dc) against the truth model t: the worst over every
    A-scan and band, and over every bin.  A zero tolerance demands equality (ratio 0, else inf); NaN is inf."""
    tol = stage_error(N) * t["norm"]                                     # (groups, M, R, ascans)
    e = np.abs(np.asarray(got).astype(np.complex128) - t["bands"])
    row = np.sqrt((e * e).sum(-1))
    out = []
    with np.errstate(all="ignore"):
        for d, tl in ((row, tol), (e, tol[..., None])):
            r = np.where(tl > 0, d / tl, np.where(d == 0, 0.0, np.inf))
            out.append(float(np.where(np.isnan(r), np.inf, r).max()))
    return tuple(out)


def check_bands(got, t, f, N, what):
    """Holds out_bands to the truth by the adjudication; t, f: the truth and float models.  Prints first.  Returns the ratios."""
    g_row, g_bin = band_ratios(got, t, N)
    o_row, o_bin = band_ratios(f["bands"], t, N)
    print("%s: bands |gpu - truth| / tol: row %.4g (f32 composition %.4g), bin %.4g (f32 composition %.4g)" % (what, g_row, o_row, g_bin, o_bin))
    RATIOS.append((what, g_row, o_row, g_bin, o_bin))
    tid = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    helpers.TRUTH_LOG.append((tid, what + " band rows", g_row, o_row))
    helpers.TRUTH_LOG.append((tid, what + " band bins", g_bin, o_bin))
    assert g_row <= max(helpers.TRUTH_LIMIT, o_row), "%s: rows: |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 composition's own %.3g)" % (what, g_row, helpers.TRUTH_LIMIT, o_row)
    assert g_bin <= max(helpers.TRUTH_LIMIT, o_bin), "%s: bins: |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 composition's own %.3g)" % (what, g_bin, helpers.TRUTH_LIMIT, o_bin)
    return g_row, o_row, g_bin, o_bin
