"""The specification of the angiography stage (include/fdoct_angio.h) in numpy, and the rule the library is held to.

The quantity.  X[g][n][r][b]: groups x repeats frames of ascans x depths complex A-scans; I = |X|^2, A = sqrt(I), N = repeats,
T[n] = X[n + 1] conj(X[n]) for the pairs n = 0 .. N - 2.
    bulk          B[g][n][r] = sum of T[n] over b in [first, first + count) (count 0: up to depths); T' = T conj(B) / |B|, and
                  T' = T where |B| = 0.  Without it T' = T.  Only cdecorr reads it.
    window        sum_win: the box [r - (wa - 1) // 2, r + wa // 2] x [b - (wd - 1) // 2, b + wd // 2], truncated to the image; cnt terms.
    var           (1 / cnt) sum_win V,  V = (1 / N) sum_n (I_n - mean_n I)^2
    decorr        1 - (1 / (N - 1)) sum_n Q_n,  Q_n = sum_win A_n A_{n+1} / sum_win (I_n + I_{n+1}) / 2,  Q_n = 1 where that is 0 / 0
    cdecorr       1 - |sum_n sum_win T'| / sum_n sum_win (I_n + I_{n+1}) / 2,  0 where the denominator is 0
    power         (1 / (N cnt)) sum_n sum_win I_n;  var, decorr and cdecorr are 0 where min_power > 0 and power < min_power.

model(..., truth=False) is the float32 composition in the kernels' order: the products, Welford's recurrence over n in increasing
n, the sums over n per pixel before the window sums, the window sums depth first then rows in increasing index from 0 with zeros
outside the image.  (The bulk sum alone is taken in numpy's order, not the kernel's strided partials and tree: any order lies
within tol_B below.)  model(..., truth=True) is everything in double from the definitions -- np.var, no recurrence.  brute() is
the definitions as plain loops per pixel over the truncated window, the check of both.

The tolerance, u = 2^-24, first order in u, from the truth alone.  Write s_win f for sum_win f.
  I             two float products and a sum: within 3 u I.
  power         N terms per pixel, cnt terms in the window, all positive, one division:
                    tol_power = (N + cnt + 4) u power.
  var           the terms' errors move V by at most (2 / N) sum_n |I_n - Ibar| 3 u I_n <= 6 u sqrt(V) rms_n(I) (Cauchy-Schwarz).
                Welford's recurrence is an updating algorithm whose M2 is within N kappa u M2, kappa = sqrt(sum_n I_n^2 / M2) (Chan,
                Golub and LeVeque 1983, table 1): N u sqrt(V) rms_n(I) on V.  Its second-order part does not vanish with V -- the
                mean is rounded at every step, by u Ibar at most, and that enters M2 squared -- so N (2 u rms_n(I))^2 is added.
                    tol_V = (N + 8) u sqrt(V) rms_n(I) + 4 N u^2 rms_n(I)^2
                    tol_var = (1 / cnt) s_win tol_V + (cnt + 2) u var     (the window sum of positive terms, the two divisions)
  decorr        sqrt halves I's 3 u and rounds once, 2.5 u each; their product 6 u.  The numerator of Q_n, cnt positive terms, is
                within (cnt + 5) u of itself; (I_n + I_{n+1}) / 2 is within 4 u, the denominator within (cnt + 3) u; the ratio
                within (2 cnt + 9) u Q_n.  N - 1 positive terms, a division and the subtraction:
                    tol_decorr = (2 cnt + N + 10) u mean_n Q_n + 2 u |decorr|
  cdecorr       a complex float product is within 4 u |X_n| |X_{n+1}| of the exact one.  With bulk: B is a float sum of `count`
                such products, within tol_B = (count + 4) u sum_b |X_n| |X_{n+1}| (Higham 4.2), which turns the unit phasor by
                tol_B / |B| (first order); the phasor's own arithmetic -- hypotf, granted OpenCL's bound of 4 ulp = 8 u, and two
                divisions -- 12 u more; the turn is another complex product, 4 u.  N - 1 terms per pixel and cnt in the window:
                    e_S = k u s_win sum_n |T| + s_win sum_n |T| tol_B / |B|,   k = N + cnt + 4, with bulk N + cnt + 20
                The denominator D, N - 1 and cnt positive terms of 4 u each, is within (N + cnt + 4) u D.  hypotf, 8 u again, a
                division, the subtraction:
                    tol_cdecorr = e_S / D + (N + cnt + 13) u |S| / D + u |cdecorr|
                (a pair whose B is exactly 0 -- a row of zeros -- turns nothing: its term is 0).
Every tolerance is of the float value stored: there is no further rounding.

The adjudication is the project's own: |gpu - truth| / tol <= max(helpers.TRUTH_LIMIT, the float composition's own ratio), every
figure printed first and appended to helpers.TRUTH_LOG.

Exemptions, from the truth alone, each capped at 1 % of a case's pixels (tests/test_angio_cases.py asserts that):
    pixels with a pair whose denominator s_win (I_n + I_{n+1}) / 2 lies below 16 times its own tolerance (cnt + 3) u s_win + cnt
    2^-126 (the float squares underflow: in practice a window of zeros) are exempt from decorr and cdecorr;
    pixels with |power_truth - min_power| <= tol_power are exempt from the mask check: they may hold 0 or the value."""
import os

import numpy as np

import helpers

U = 2.0 ** -24
TINY = 2.0 ** -126
NAMES = ("var", "decorr", "cdecorr", "power")
TILE_ROWS, TILE_DEPTHS, BLOCKS_PER_CU = 16, 64, 4     # kBoxRows, kBoxDepths, kBoxWavesPerCu / 4 (fdoct_boxtile.h)
PLAN_CUS = 256                                        # what fdoct_angio_plan, which has no handle, takes for the card
RATIOS = []   # (what, {output: (gpu ratio, f32 ratio)}), one per check()


def bulk_range(bulk, depths):
    """(first, count) of the bulk sum, or None: bulk is None / False, True (all depths) or (first, count), count 0 meaning the rest."""
    if bulk is None or bulk is False:
        return None
    first, cnt = (0, 0) if bulk is True else bulk
    return first, cnt if cnt else depths - first


def geometry(nframes, repeats, ascans, depths, cus=PLAN_CUS):
    """(groups, tiles, workgroups) of angio_plan_launch."""
    groups = nframes // repeats
    tiles = groups * (-(-ascans // TILE_ROWS)) * (-(-depths // TILE_DEPTHS))
    return groups, tiles, min(tiles, cus * BLOCKS_PER_CU)


def _grouped(X, repeats):
    X = np.asarray(X)
    assert X.ndim == 3 and repeats >= 2 and X.shape[0] % repeats == 0
    return X.reshape(X.shape[0] // repeats, repeats, X.shape[1], X.shape[2])


def box(P, wa, wd):
    """sum_win of P (..., H, D) in P's type: zeros outside the image, depth first then rows, in increasing index from 0."""
    H, D = P.shape[-2:]
    pad = np.zeros(P.shape[:-2] + (H + wa - 1, D + wd - 1), P.dtype)
    br, bd = (wa - 1) // 2, (wd - 1) // 2
    pad[..., br:br + H, bd:bd + D] = P
    dep = np.zeros(P.shape[:-2] + (H + wa - 1, D), P.dtype)
    for j in range(wd):
        dep = dep + pad[..., j:j + D]
    out = np.zeros(P.shape, P.dtype)
    for j in range(wa):
        out = out + dep[..., j:j + H, :]
    return out


def count(H, D, wa, wd):
    """cnt (H, D): the window's overlap with the image."""
    r, b = np.arange(H), np.arange(D)
    nr = np.minimum(r + wa // 2, H - 1) - np.maximum(r - (wa - 1) // 2, 0) + 1
    nb = np.minimum(b + wd // 2, D - 1) - np.maximum(b - (wd - 1) // 2, 0) + 1
    return nr[:, None] * nb[None, :]


def _mask(out, min_power):
    if min_power > 0:
        below = out["power"] < min_power
        for k in ("var", "decorr", "cdecorr"):
            out[k] = np.where(below, 0, out[k]).astype(out[k].dtype)
    return out


def _lag(xr, xi, rng, f):
    """T' (re, im) in type f, |T|, and B (complex) with the bulk range rng."""
    re = xr[:, 1:] * xr[:, :-1] + xi[:, 1:] * xi[:, :-1]
    im = xi[:, 1:] * xr[:, :-1] - xr[:, 1:] * xi[:, :-1]
    if not rng:
        return re, im, None
    first, cnt = rng
    Br, Bi = re[..., first:first + cnt].sum(-1, dtype=f), im[..., first:first + cnt].sum(-1, dtype=f)
    m = np.hypot(Br, Bi).astype(f)
    ok = m > 0
    ux = np.where(ok, Br / np.where(ok, m, 1), 1).astype(f)[..., None]
    uy = np.where(ok, -(Bi / np.where(ok, m, 1)), 0).astype(f)[..., None]
    return re * ux - im * uy, re * uy + im * ux, Br + 1j * Bi


def _composition(Xg, wa, wd, rng, min_power):
    f = np.float32
    G, N, H, D = Xg.shape
    xr, xi = Xg.real.astype(f), Xg.imag.astype(f)
    I = xr * xr + xi * xi
    cnt = count(H, D, wa, wd)
    sum_i, mean, m2 = np.zeros((G, H, D), f), np.zeros((G, H, D), f), np.zeros((G, H, D), f)
    for n in range(N):
        sum_i = sum_i + I[:, n]
        delta = I[:, n] - mean
        mean = mean + delta / f(n + 1)
        m2 = m2 + delta * (I[:, n] - mean)
    tre, tim, _ = _lag(xr, xi, rng, f)
    s_re, s_im, s_half, q = np.zeros((G, H, D), f), np.zeros((G, H, D), f), np.zeros((G, H, D), f), np.zeros((G, H, D), f)
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(N - 1):
            hh = f(0.5) * (I[:, n] + I[:, n + 1])
            s_re, s_im, s_half = s_re + tre[:, n], s_im + tim[:, n], s_half + hh
            num, den = box(np.sqrt(I[:, n]) * np.sqrt(I[:, n + 1]), wa, wd), box(hh, wa, wd)
            q = q + np.where(den == 0, f(1), num / np.where(den == 0, f(1), den)).astype(f)
        w_half = box(s_half, wa, wd)
        mag = np.hypot(box(s_re, wa, wd), box(s_im, wa, wd)).astype(f)
        out = dict(var=box(m2 / f(N), wa, wd) / cnt.astype(f), decorr=f(1) - q / f(N - 1),
                   cdecorr=np.where(w_half == 0, f(0), f(1) - mag / np.where(w_half == 0, f(1), w_half)).astype(f),
                   power=box(sum_i, wa, wd) / (N * cnt).astype(f))
    assert all(v.dtype == f for v in out.values())
    return _mask(out, f(min_power))


def _truth(Xg, wa, wd, rng, min_power):
    Xg = np.asarray(Xg, np.complex128)
    G, N, H, D = Xg.shape
    I = Xg.real ** 2 + Xg.imag ** 2
    A = np.abs(Xg)
    cnt = count(H, D, wa, wd).astype(np.float64)
    tre, tim, B = _lag(Xg.real, Xg.imag, rng, np.float64)
    half = 0.5 * (I[:, :-1] + I[:, 1:])
    num, den = box(A[:, :-1] * A[:, 1:], wa, wd), box(half, wa, wd)           # (G, N - 1, H, D)
    Q = np.where(den == 0, 1.0, num / np.where(den == 0, 1.0, den))
    S = box(tre.sum(1), wa, wd) + 1j * box(tim.sum(1), wa, wd)
    Dn = den.sum(1)
    out = dict(var=box(I.var(1), wa, wd) / cnt, decorr=1.0 - Q.mean(1), cdecorr=np.where(Dn == 0, 0.0, 1.0 - np.abs(S) / np.where(Dn == 0, 1.0, Dn)),
               power=box(I.sum(1), wa, wd) / (N * cnt))
    out = _mask(out, min_power)
    out.update(Q=Q, den=den, S=S, D=Dn, B=B, cnt=cnt)
    return out


def model(X, repeats, win=(1, 1), bulk=None, min_power=0.0, truth=False):
    """dict(var, decorr, cdecorr, power), each (groups, H, D): float32, or float64 with truth (which also returns Q and den per pair,
    S, D, B and cnt)."""
    Xg = _grouped(X, repeats)
    rng = bulk_range(bulk, Xg.shape[3])
    return _truth(Xg, win[0], win[1], rng, min_power) if truth else _composition(Xg, win[0], win[1], rng, min_power)


def brute(X, repeats, win=(1, 1), bulk=None):
    """The four outputs by the definitions, pixel by pixel in double over the truncated window (no mask)."""
    Xg = np.asarray(_grouped(X, repeats), np.complex128)
    G, N, H, D = Xg.shape
    wa, wd = win
    rng = bulk_range(bulk, D)
    out = {k: np.zeros((G, H, D)) for k in NAMES}
    for g in range(G):
        T = Xg[g, 1:] * np.conj(Xg[g, :-1])
        if rng:
            B = T[..., rng[0]:rng[0] + rng[1]].sum(-1)
            m = np.abs(B)
            T = T * np.where(m > 0, np.conj(B) / np.where(m > 0, m, 1), 1)[..., None]
        I = np.abs(Xg[g]) ** 2
        for r in range(H):
            r0, r1 = max(r - (wa - 1) // 2, 0), min(r + wa // 2, H - 1) + 1
            for b in range(D):
                b0, b1 = max(b - (wd - 1) // 2, 0), min(b + wd // 2, D - 1) + 1
                w = I[:, r0:r1, b0:b1]
                cnt = w[0].size
                out["power"][g, r, b] = w.sum() / (N * cnt)
                out["var"][g, r, b] = ((w - w.mean(0)) ** 2).mean(0).sum() / cnt
                qs = 0.0
                for n in range(N - 1):
                    den = 0.5 * (w[n] + w[n + 1]).sum()
                    qs += 1.0 if den == 0 else np.sqrt(w[n] * w[n + 1]).sum() / den
                out["decorr"][g, r, b] = 1.0 - qs / (N - 1)
                Dn = 0.5 * (w[:-1] + w[1:]).sum()
                out["cdecorr"][g, r, b] = 0.0 if Dn == 0 else 1.0 - abs(T[:, r0:r1, b0:b1].sum()) / Dn
    return out


def tolerances(X, repeats, win=(1, 1), bulk=None, min_power=0.0):
    """dict(var, decorr, cdecorr, power (groups, H, D), den_tol (groups, N - 1, H, D), truth) from the truth alone."""
    Xg = np.asarray(_grouped(X, repeats), np.complex128)
    G, N, H, D = Xg.shape
    wa, wd = win
    rng = bulk_range(bulk, D)
    tr = _truth(Xg, wa, wd, rng, 0.0)
    cnt = tr["cnt"]
    I = Xg.real ** 2 + Xg.imag ** 2
    rms_i = np.sqrt((I * I).mean(1))
    V = I.var(1)
    tol_V = (N + 8) * U * np.sqrt(V) * rms_i + 4 * N * U * U * rms_i * rms_i
    mag = np.abs(Xg[:, :-1]) * np.abs(Xg[:, 1:])                           # |T|, (G, N - 1, H, D)
    k = N + cnt + (20 if rng else 4)
    e_S = k * U * box(mag.sum(1), wa, wd)
    if rng:
        first, c = rng
        tol_B = (c + 4) * U * mag[..., first:first + c].sum(-1)
        live = tol_B > 0
        turn = np.where(live, tol_B / np.where(live, np.maximum(np.abs(tr["B"]), 1e-300), 1), 0)
        e_S = e_S + box((mag * turn[..., None]).sum(1), wa, wd)
    Dn = tr["D"]
    safe = np.where(Dn == 0, 1.0, Dn)
    return dict(truth=tr,
                power=(N + cnt + 4) * U * tr["power"],
                var=box(tol_V, wa, wd) / cnt + (cnt + 2) * U * tr["var"],
                decorr=(2 * cnt + N + 10) * U * tr["Q"].mean(1) + 2 * U * np.abs(tr["decorr"]),
                cdecorr=e_S / safe + (N + cnt + 13) * U * np.abs(tr["S"]) / safe + U * np.abs(tr["cdecorr"]),
                den_tol=(cnt + 3) * U * tr["den"] + cnt * TINY)


def exemptions(X, repeats, win=(1, 1), bulk=None, min_power=0.0, tol=None):
    """(pixels exempt from decorr and cdecorr; pixels exempt from the mask check) as boolean (groups, H, D) arrays, from the truth alone."""
    tol = tol or tolerances(X, repeats, win, bulk, min_power)
    tr = tol["truth"]
    ill = (tr["den"] < 16 * tol["den_tol"]).any(1)
    edge = np.abs(tr["power"] - min_power) <= tol["power"] if min_power > 0 else np.zeros(ill.shape, bool)
    return ill, edge


def _ratio(got, ref, tol, keep, edge=None):
    """Worst |got - ref| / tol over the pixels kept; at the mask's edge 0 will do as well as ref.  A pixel whose tolerance is 0 must
    be exact."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    if edge is not None:
        err = np.where(edge, np.minimum(err, np.abs(got)), err)
    with np.errstate(divide="ignore", invalid="ignore"):
        rat = np.where(err == 0, 0.0, err / tol)
    return float(rat[keep].max()) if np.any(keep) else 0.0


def check(gpu, X, what, repeats, win=(1, 1), bulk=None, min_power=0.0, refs=None):
    """gpu: dict of any of var, decorr, cdecorr, power as the library wrote them.  Every output against the truth by the
    adjudication, the mask exactly; every figure printed before anything is asserted.  refs: (model, truth, tolerances,
    exemptions) where the caller has them already."""
    kw = dict(repeats=repeats, win=win, bulk=bulk, min_power=min_power)
    if refs is None:
        tol = tolerances(X, **kw)
        refs = (model(X, **kw), model(X, truth=True, **kw), tol, exemptions(X, tol=tol, **kw))
    f32, tr, tol, (ill, edge) = refs
    names = [k for k in NAMES if k in gpu and gpu[k] is not None]
    for k in names:
        g = np.asarray(gpu[k])
        assert g.dtype == np.float32 and g.shape == tr[k].shape, (what, k, g.dtype, g.shape)
        assert np.isfinite(g).all(), what + ": %s is not finite (an output pixel was not written)" % k
    every = np.ones(ill.shape, bool)
    if min_power > 0:
        below, above = (tol["truth"]["power"] < min_power) & ~edge, (tol["truth"]["power"] >= min_power) & ~edge
    else:
        below, above = ~every, every
    figs, unmasked = {}, 0
    for k in names:
        if k == "power":
            figs[k] = (_ratio(gpu[k], tr[k], tol[k], every), _ratio(f32[k], tr[k], tol[k], every))
            continue
        want = np.where(below, 0, tol["truth"][k])     # the truth's value, 0 below the mask, either at its edge
        keep = every if k == "var" else ~ill
        figs[k] = (_ratio(gpu[k], want, tol[k], keep, edge), _ratio(f32[k], want, tol[k], keep, edge))
        unmasked += int(np.count_nonzero(np.asarray(gpu[k])[below]))
    print("%s: |gpu - truth| / tol (f32 model) %s; %d of %d pixels exempt, %d at the mask's edge, %d masked of which %d not 0" % (
        what, ", ".join("%s %.4f (%.4f)" % (k, figs[k][0], figs[k][1]) for k in names), int(ill.sum()), ill.size, int(edge.sum()), int(below.sum()),
        unmasked))
    RATIOS.append((what, figs))
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    for k in names:
        helpers.TRUTH_LOG.append((test, "%s (angio %s)" % (what, k), figs[k][0], figs[k][1]))
    for k in names:
        g, o = figs[k]
        assert g <= max(helpers.TRUTH_LIMIT, o), "%s: %s |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 model's own %.3g)" % (
            what, k, g, helpers.TRUTH_LIMIT, o)
    assert unmasked == 0, "%s: %d values below min_power are not 0" % (what, unmasked)
    if min_power > 0 and "power" in names and above.any():   # all 0 would be a mask over everything
        others = [k for k in names if k != "power"]
        assert not others or any(np.count_nonzero(np.asarray(gpu[k])[above]) > 0 for k in others), what + ": every pixel above min_power is 0"
    return figs
