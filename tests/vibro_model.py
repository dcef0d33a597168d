"""The specification of the vibrometry stage (include/fdoct_vibro.h) in numpy, and the rule the library is held to.

The quantity.  X[t][r][b]: T frames of ascans x depths complex A-scans; time is the frame index.
    reference     C[t][r] = sum of X[t][r][b] over b in [first, first + count) (count 0: up to depths); Y = X conj(C) / |C|, and
                  Y = X where |C| = 0.  Without it Y = X.
    steps         d[s] = angle(Y[s + 1] conj(Y[s])), s = 0 .. T - 2.
    phase         phi[0] = 0, phi[t] = phi[t - 1] + d[t - 1]: np.unwrap of angle(Y) over t, counted from its first value.
    detrend       0: phi' = phi - mean(phi);  1: phi' = phi - (alpha + beta t), the least-squares line.
    window        w = 1 (RECT) or 0.5 - 0.5 cos(2 pi t / (T - 1)) (HANN; 1 for T = 2).
    lock-in       A_j = (2 / sum w) sum_t w[t] phi'[t] exp(-2 pi i nu_j t).
    outputs       amp = scale A;  rms = |scale| sqrt(mean phi'^2);  drift = scale phi[T - 1];  power = mean |X|^2;  amp, rms and
                  drift are 0 where min_power > 0 and power < min_power.

model(..., truth=False) is the float / double composition in the kernels' order: float32 products, reference sum and arctan2;
phi and every sum over time in double, chunk by chunk from the chunk's own start, the chunks put together by the identities of
fdoct_vibro.hip, the mean or the line removed through the closed forms.  model(..., truth=True) is everything in double by the
definition itself -- no chunks, no closed forms.  brute() is the definition as plain loops per pixel with np.unwrap, the check of
both.

The tolerance, u = 2^-24.
  per step      The lag product's components are each two float products and a sum: the product is within 4 u |Y[s]| |Y[s + 1]|
                of the exact one, which turns its angle by at most 4 u; the turn by the reference phasor is such a product too.
                8 u covers both.  arctan2f itself: PHASE_STEP = 4 ATAN2F_HOST, ATAN2F_HOST the worst |float32 arctan2 - float64
                arctan2| on the float composition's own lag products over every case of tests/vibro_cases.py, measured on the
                CPU: 2.96e-07 rad (the ramp of 2.5 rad a frame, angles near pi; the others 1.3e-07 .. 2.8e-07), recorded below as
                3.0e-07; tests/test_vibro_cases.py prints each case's figure and asserts it does not exceed the record.  The
                device's libm is granted four times the host's: PHASE_STEP = 1.2e-06 rad.  With a reference, C is a float sum of `count` terms: within tol_C =
                (count + 4) u sum |X| of the exact sum over the range (Higham 4.2), which turns the unit phasor by at most
                tol_C / |C| (first order; the cases keep |C| >= 16 tol_C), at both ends of the step.  So
                    e_s = PHASE_STEP + 8 u + tol_C[s] / |C[s]| + tol_C[s + 1] / |C[s + 1]|
                (the last two with a reference only, and 0 for a row of zeros, where C = 0 and Y = X = 0 exactly).
  per pixel     phi[t] is off by at most E[t] = sum of e_s over s < t.  Both detrends are orthogonal projections in R^T, which
                do not lengthen a vector, so ||phi'_gpu - phi'_truth||_2 <= ||E||_2 and
                    tol_rms   = |scale| sqrt(mean E^2)                     (the reverse triangle inequality on the norm)
                    tol_amp   = |scale| (2 / sum w) ||w||_2 ||E||_2        (Cauchy-Schwarz, |e^(i x)| = 1)
                    tol_drift = |scale| E[T - 1]
                    tol_power = (T + 4) u power                            (float squares, a double sum)
                Each output is written as a float: u |value| is added for that last rounding.
  double        The sums over time are double sums of at most T terms each, the chunk identities add four terms a chunk, and
                the closed forms subtract: RSS = S2 - S1 mean - beta Stc cancels, and so does sum w phi e - alpha G0 - beta G1.
                With v = 2^-53 and k = T + 8 + 4 chunks:
                    |dRSS| <= k v (S2 + |S1 mean| + |beta Stc|), and |sqrt(a + d) - sqrt(a)| <= min(sqrt|d|, |d| / sqrt(a)), so
                    rms term = |scale| min(sqrt(dRSS / T), dRSS / (T rms_truth))
                    amp term = |scale| (2 / sum w) (k v (sum w |phi| + |alpha| sum w + |beta| sum w t) + 4 pi T v sum w |phi'|)
                (the second part: 2 nu t is rounded once before sincospi, which moves the angle by at most 2 pi T v, and numpy's
                own cos and sin of 2 pi nu t as much again).  tests/test_vibro_cases.py shows both below 1/16 of the float term
                on every case; they are added to it all the same.

The adjudication is the project's own: |gpu - truth| / tol <= max(helpers.TRUTH_LIMIT, the float composition's own ratio), every
figure printed first and appended to helpers.TRUTH_LOG.

Exemptions, from the truth alone, each capped at 1 % of a case's pixels (tests/test_vibro_cases.py asserts that):
    pixels with a step where pi - |d_truth| < 16 e_s (the wrap may flip), or where |Y[s]| |Y[s + 1]| < 16 (4 u |Y[s]| |Y[s + 1]| +
    2^-126) (the product underflows its conditioning: in practice a frame of zeros) are exempt from amp, rms and drift;
    pixels with |power_truth - min_power| <= tol_power are exempt from the mask check: they may hold 0 or the value."""
import os

import numpy as np

import helpers

U = 2.0 ** -24
V = 2.0 ** -53
ATAN2F_HOST = 3.0e-07                     # rad; measured 2.96e-07 (see above)
PHASE_STEP = 4 * ATAN2F_HOST              # rad
RECT, HANN = 0, 1
TARGET_WAVES, MIN_CHUNK = 1024, 64        # kVibTargetWaves, kVibMinChunk (fdoct_vibro_kernels.h)
RATIOS = []   # (what, {output: (gpu ratio, f32 ratio)}), one per check()


def ref_range(ref, depths):
    """(first, count) of the reference sum, or None: ref is None / False, True (all depths) or (first, count), count 0 meaning the rest."""
    if ref is None or ref is False:
        return None
    first, cnt = (0, 0) if ref is True else ref
    return first, cnt if cnt else depths - first


def window(kind, T):
    t = np.arange(T, dtype=np.float64)
    return np.ones(T) if kind == RECT or T <= 2 else 0.5 - 0.5 * np.cos(2 * np.pi * t / (T - 1))


def chunk_rule(T, pixels):
    """fdoct_vibro_plan's rule: chunk_steps from (T, pixels)."""
    waves = (pixels + 63) // 64
    want = (TARGET_WAVES + waves - 1) // waves
    return min(max(-(-(T - 1) // want), MIN_CHUNK), T - 1)


def chunks_of(T, chunk_steps):
    """[(t0, t1)]: chunk c reads frames t0 .. t1 and owns samples t0 + 1 .. t1."""
    cs = min(chunk_steps, T - 1)
    return [(t0, min(t0 + cs, T - 1)) for t0 in range(0, T - 1, cs)]


def table(freq, kind, T):
    """(nfreq, T) complex128: w (cos + i sin)(2 pi nu t)."""
    t = np.arange(T, dtype=np.float64)
    w = window(kind, T)
    return np.array([w * np.exp(2j * np.pi * nu * t) for nu in freq], np.complex128).reshape(len(freq), T)


def _reference(X, ref, f):
    """Y (as re, im in type f) and C (complex, or None)."""
    xr, xi = X.real.astype(f), X.imag.astype(f)
    rng = ref_range(ref, X.shape[2])
    if not rng:
        return xr, xi, None
    first, cnt = rng
    Cr, Ci = xr[..., first:first + cnt].sum(-1, dtype=f), xi[..., first:first + cnt].sum(-1, dtype=f)   # any order is within tol_C
    m = np.hypot(Cr, Ci).astype(f)
    ok = m != 0
    ur = np.where(ok, Cr / np.where(ok, m, 1), 1).astype(f)[..., None]
    ui = np.where(ok, -Ci / np.where(ok, m, 1), 0).astype(f)[..., None]
    return xr * ur - xi * ui, xr * ui + xi * ur, Cr + 1j * Ci


def steps(X, ref, truth=False):
    """d (T - 1, H, D) float64, and the lag product's (re, im) it is the angle of."""
    f = np.float64 if truth else np.float32
    yr, yi, _ = _reference(np.asarray(X), ref, f)
    re, im = yr[1:] * yr[:-1] + yi[1:] * yi[:-1], yi[1:] * yr[:-1] - yr[1:] * yi[:-1]
    return np.arctan2(im, re).astype(np.float64), re, im


def _mask(out, power, min_power):
    if min_power > 0:
        below = power < min_power
        out["amp"] = np.where(below[None], 0, out["amp"])
        out["rms"], out["drift"] = np.where(below, 0, out["rms"]), np.where(below, 0, out["drift"])
    return out


def _truth(X, freq, ref, detrend, kind, scale, min_power):
    X = np.asarray(X, np.complex128)
    T = X.shape[0]
    d, _, _ = steps(X, ref, truth=True)
    phi = np.concatenate([np.zeros((1,) + d.shape[1:]), np.cumsum(d, 0)], 0)
    t = np.arange(T, dtype=np.float64)
    if detrend:
        tc = t - t.mean()
        beta = np.tensordot(tc, phi, 1) / (tc * tc).sum()
        res = phi - phi.mean(0) - tc[:, None, None] * beta
    else:
        res = phi - phi.mean(0)
    w = window(kind, T)
    e = np.conj(table(freq, kind, T))                                   # w exp(-2 pi i nu t)
    amp = np.tensordot(e, res, 1) * (2.0 / w.sum()) if len(freq) else np.zeros((0,) + phi.shape[1:], np.complex128)
    power = (X.real ** 2 + X.imag ** 2).mean(0)
    out = dict(amp=scale * amp, rms=abs(scale) * np.sqrt((res * res).mean(0)), drift=scale * phi[-1], power=power, phi=phi, res=res, d=d)
    return _mask(out, power, min_power)


def _composition(X, freq, ref, detrend, kind, scale, min_power, chunk_steps):
    X = np.asarray(X)
    T, H, D = X.shape
    nf = len(freq)
    d, _, _ = steps(X, ref)
    xr, xi = X.real.astype(np.float32), X.imag.astype(np.float32)
    pw = (xr * xr + xi * xi).astype(np.float64)
    tab = table(freq, kind, T)
    w = window(kind, T)
    z = lambda *s: np.zeros(s + (H, D))   # noqa: E731
    S1, S2, St, P, Sc, Ss, off = z(), z(), z(), z(), z(nf), z(nf), z()
    G0, G1, SW = tab[:, 0].copy(), np.zeros(nf, np.complex128), w[0]
    for c, (t0, t1) in enumerate(chunks_of(T, chunk_steps)):
        s1, s2, st, p, sc, ss, phi = z(), z(), z(), z(), z(nf), z(nf), z()
        if c == 0:
            p += pw[0]
        for t in range(t0 + 1, t1 + 1):
            p += pw[t]
            phi = phi + d[t - 1]
            s1 += phi
            s2 += phi * phi
            st += float(t) * phi
            for j in range(nf):
                sc[j] += tab[j, t].real * phi
                ss[j] += tab[j, t].imag * phi
        nc, sum_t = float(t1 - t0), float((t1 - t0) * (t0 + 1 + t1) // 2)
        E, F = tab[:, t0 + 1:t1 + 1].sum(1), (tab[:, t0 + 1:t1 + 1] * np.arange(t0 + 1, t1 + 1)).sum(1)
        S1 += s1 + nc * off
        S2 += (s2 + (2.0 * off) * s1) + (nc * off) * off
        St += st + off * sum_t
        P += p
        for j in range(nf):
            Sc[j] += sc[j] + off * E[j].real
            Ss[j] += ss[j] + off * E[j].imag
        off = off + phi
        G0, G1, SW = G0 + E, G1 + F, SW + w[t0 + 1:t1 + 1].sum()
    n = float(T)
    power = P / n
    mean = S1 / n
    alpha, beta, rss = mean, np.zeros_like(mean), S2 - S1 * mean
    if detrend:
        tbar, stt = 0.5 * (n - 1.0), n * (n * n - 1.0) / 12.0
        stc = St - tbar * S1
        beta = stc / stt
        alpha = mean - beta * tbar
        rss = rss - beta * stc
    rss = np.where(rss < 0, 0.0, rss)
    k = 2.0 * scale / SW
    amp = np.zeros((nf, H, D), np.complex64)
    for j in range(nf):
        re = Sc[j] - alpha * G0[j].real - beta * G1[j].real
        im = Ss[j] - alpha * G0[j].imag - beta * G1[j].imag
        amp[j] = (k * re).astype(np.float32) + 1j * (-(k * im)).astype(np.float32)
    out = dict(amp=amp, rms=(abs(scale) * np.sqrt(rss / n)).astype(np.float32), drift=(scale * off).astype(np.float32), power=power.astype(np.float32))
    return _mask(out, power, min_power)


def model(X, freq=(), ref=None, detrend=0, window=RECT, scale=1.0, min_power=0.0, chunk_steps=0, truth=False):
    """dict(amp (nfreq, H, D), rms, drift, power (H, D)): complex64 / float32, or complex128 / float64 with truth (which also
    returns phi, its residual res and the steps d)."""
    X = np.asarray(X)
    assert X.ndim == 3 and X.shape[0] >= 2
    if truth:
        return _truth(X, freq, ref, detrend, window, scale, min_power)
    cs = chunk_steps if chunk_steps else chunk_rule(X.shape[0], X.shape[1] * X.shape[2])
    return _composition(X, freq, ref, detrend, window, scale, min_power, cs)


def brute(X, freq=(), ref=None, detrend=0, window=RECT, scale=1.0):
    """amp, rms, drift and power by the definition, pixel by pixel in double (no mask)."""
    X = np.asarray(X, np.complex128)
    T, H, D = X.shape
    rng = ref_range(ref, D)
    t = np.arange(T, dtype=np.float64)
    w = globals()["window"](window, T)
    amp, rms, drift, power = np.zeros((len(freq), H, D), np.complex128), np.zeros((H, D)), np.zeros((H, D)), np.zeros((H, D))
    for r in range(H):
        Y = X[:, r, :]
        if rng:
            C = Y[:, rng[0]:rng[0] + rng[1]].sum(1)
            m = np.abs(C)
            Y = Y * np.where(m > 0, np.conj(C) / np.where(m > 0, m, 1), 1)[:, None]
        for b in range(D):
            a = np.angle(Y[:, b])
            phi = np.unwrap(a) - a[0]
            res = phi - np.polyval(np.polyfit(t, phi, 1), t) if detrend and T > 2 else phi - phi.mean()
            if detrend and T == 2:
                res = np.zeros(2)
            for j, nu in enumerate(freq):
                amp[j, r, b] = scale * (2.0 / w.sum()) * (w * res * np.exp(-2j * np.pi * nu * t)).sum()
            rms[r, b], drift[r, b], power[r, b] = abs(scale) * np.sqrt((res * res).mean()), scale * phi[-1], (np.abs(X[:, r, b]) ** 2).mean()
    return dict(amp=amp, rms=rms, drift=drift, power=power)


def tolerances(X, freq=(), ref=None, detrend=0, window=RECT, scale=1.0, min_power=0.0, chunk_steps=0):
    """dict(amp (H, D), rms, drift, power, e (T - 1, H, D), float and double parts, tol_C, C) from the truth alone."""
    X = np.asarray(X, np.complex128)
    T, H, D = X.shape
    tr = _truth(X, freq, ref, detrend, window, scale, 0.0)
    mag = np.abs(X)
    e = np.full((T - 1, H, D), PHASE_STEP + 8 * U)
    out = {}
    rng = ref_range(ref, D)
    if rng:
        first, cnt = rng
        C = X[..., first:first + cnt].sum(-1)
        tol_C = (cnt + 4) * U * mag[..., first:first + cnt].sum(-1)
        live = tol_C > 0
        turn = np.where(live, tol_C / np.where(live, np.abs(C), 1), 0)
        e = e + (turn[:-1] + turn[1:])[..., None]
        out.update(C=C, tol_C=tol_C)
    E = np.concatenate([np.zeros((1, H, D)), np.cumsum(e, 0)], 0)
    w = globals()["window"](window, T)
    s = abs(scale)
    E2 = np.sqrt((E * E).sum(0))
    f_rms, f_amp, f_drift = s * np.sqrt((E * E).mean(0)), s * (2.0 / w.sum()) * np.sqrt((w * w).sum()) * E2, s * E[-1]
    # the double arithmetic's own term
    cs = chunk_steps if chunk_steps else chunk_rule(T, H * D)
    k = T + 8 + 4 * len(chunks_of(T, cs))
    phi, res = tr["phi"], tr["res"]
    t = np.arange(T, dtype=np.float64)
    S1, S2 = phi.sum(0), (phi * phi).sum(0)
    mean = S1 / T
    tc = t - t.mean()
    stc = np.tensordot(tc, phi, 1)
    beta = stc / max((tc * tc).sum(), 1e-300) if detrend else np.zeros((H, D))
    alpha = mean - beta * t.mean()
    dRSS = k * V * (S2 + np.abs(S1 * mean) + np.abs(beta * stc))
    rms_t = np.sqrt((res * res).mean(0))
    d_rms = s * np.minimum(np.sqrt(dRSS / T), dRSS / (T * np.where(rms_t > 0, rms_t, 1e-300)))
    wphi, wres = np.tensordot(w, np.abs(phi), 1), np.tensordot(w, np.abs(res), 1)
    d_amp = s * (2.0 / w.sum()) * (k * V * (wphi + np.abs(alpha) * w.sum() + np.abs(beta) * (w * t).sum()) + 4 * np.pi * T * V * wres)
    amp_mag = np.abs(tr["amp"]).max(0) if len(freq) else np.zeros((H, D))
    out.update(truth=tr, e=e, f_rms=f_rms, f_amp=f_amp, f_drift=f_drift, d_rms=d_rms, d_amp=d_amp,
               rms=f_rms + d_rms + U * tr["rms"], amp=f_amp + d_amp + U * amp_mag, drift=f_drift + U * np.abs(tr["drift"]),
               power=(T + 4) * U * tr["power"])
    return out


def exemptions(X, freq=(), ref=None, detrend=0, window=RECT, scale=1.0, min_power=0.0, chunk_steps=0, tol=None):
    """(pixels exempt from amp, rms and drift; pixels exempt from the mask check) as boolean (H, D) arrays, from the truth alone."""
    X = np.asarray(X, np.complex128)
    tol = tol or tolerances(X, freq, ref, detrend, window, scale, min_power, chunk_steps)
    yr, yi, _ = _reference(X, ref, np.float64)
    d = np.arctan2(yi[1:] * yr[:-1] - yr[1:] * yi[:-1], yr[1:] * yr[:-1] + yi[1:] * yi[:-1])
    prod = np.hypot(yr, yi)[1:] * np.hypot(yr, yi)[:-1]
    ill = ((np.pi - np.abs(d) < 16 * tol["e"]) | (prod < 16 * (4 * U * prod + 2.0 ** -126))).any(0)
    power = (X.real ** 2 + X.imag ** 2).mean(0)
    edge = np.abs(power - min_power) <= tol["power"] if min_power > 0 else np.zeros(ill.shape, bool)
    return ill, edge


def _ratio(got, ref, tol, keep, edge=None):
    """Worst |got - ref| / tol over the pixels kept (tol > 0 there); at the mask's edge 0 will do as well as ref."""
    got = np.asarray(got, np.complex128)
    err = np.abs(got - ref)
    if edge is not None:
        err = np.where(np.broadcast_to(edge, err.shape), np.minimum(err, np.abs(got)), err)
    keep = np.broadcast_to(keep, err.shape)
    return float((err / np.broadcast_to(tol, err.shape))[keep].max()) if keep.any() else 0.0


def check(gpu, X, what, freq=(), ref=None, detrend=0, window=RECT, scale=1.0, min_power=0.0, chunk_steps=0, refs=None):
    """gpu: dict(amp, rms, drift, power) as the library wrote them (amp may be absent without frequencies).  Every output
    against the truth by the adjudication, the mask exactly; every figure printed before anything is asserted.  refs: (model,
    truth, tolerances, exemptions) where the caller has them already."""
    kw = dict(freq=freq, ref=ref, detrend=detrend, window=window, scale=scale, min_power=min_power, chunk_steps=chunk_steps)
    if refs is None:
        tol = tolerances(X, **kw)
        refs = (model(X, **kw), model(X, truth=True, **kw), tol, exemptions(X, tol=tol, **kw))
    f32, tr, tol, (ill, edge) = refs
    names = [k for k in ("amp", "rms", "drift", "power") if k in gpu and gpu[k] is not None]
    for k in names:
        g = np.asarray(gpu[k])
        assert g.dtype == (np.complex64 if k == "amp" else np.float32) and g.shape == tr[k].shape, (what, k, g.dtype, g.shape)
        assert np.isfinite(g.view(np.float32)).all(), what + ": %s is not finite (an output pixel was not written)" % k
    if min_power > 0:
        below, above = (tr["power"] < min_power) & ~edge, (tr["power"] >= min_power) & ~edge
    else:
        below, above = np.zeros(ill.shape, bool), np.ones(ill.shape, bool)
    figs, unmasked = {}, 0
    for k in names:
        if k == "power":
            figs[k] = (_ratio(gpu[k], tr[k], tol[k], True), _ratio(f32[k], tr[k], tol[k], True))
        else:   # the truth's value, 0 below the mask, either at its edge
            want = np.where(below, 0, tol["truth"][k])
            figs[k] = (_ratio(gpu[k], want, tol[k], ~ill, edge), _ratio(f32[k], want, tol[k], ~ill, edge))
        if k != "power":
            unmasked += int(np.count_nonzero(np.asarray(gpu[k])[..., below]))
    print("%s: |gpu - truth| / tol (f32 model) %s; %d of %d pixels exempt, %d at the mask's edge, %d masked of which %d not 0" % (
        what, ", ".join("%s %.4f (%.4f)" % (k, figs[k][0], figs[k][1]) for k in names), int(ill.sum()), ill.size, int(edge.sum()), int(below.sum()),
        unmasked))
    RATIOS.append((what, figs))
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    for k in names:
        helpers.TRUTH_LOG.append((test, "%s (vibro %s)" % (what, k), figs[k][0], figs[k][1]))
    for k in names:
        g, o = figs[k]
        assert g <= max(helpers.TRUTH_LIMIT, o), "%s: %s |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 model's own %.3g)" % (
            what, k, g, helpers.TRUTH_LIMIT, o)
    assert unmasked == 0, "%s: %d values below min_power are not 0" % (what, unmasked)
    if min_power > 0 and "rms" in names and (above & ~ill).any():   # a live pixel above the mask moves: all 0 would be a mask over everything
        assert np.count_nonzero(np.asarray(gpu["rms"])[above & ~ill]) > 0, what + ": every pixel above min_power is 0"
    return figs
