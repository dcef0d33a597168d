"""The specification of the coherent-averaging stage (include/fdoct_cxavg.h) in numpy, and the rule the library is held to.

The quantity.  X[f][r][b]: nframes frames of ascans x depths complex A-scans; N = repeats, S = stride; group g's repeat n is frame
g S + n, G = (nframes - N) / S + 1 groups; X_n is repeat n of the group at hand.
    alignment     C[g][n][r] = sum of X_n conj(X_ref) over b in [first, first + count) (count 0: up to depths); align 2 adds the
                  A-scans: C[g][n] = sum_r C[g][n][r].  U = conj(C) / |C|, 1 where |C| = 0, and exactly 1 for n = ref and with align 0.
    mean          Z = (sum_n U_n X_n) / N
    mag           |Z|
    incoh         (sum_n |X_n|) / N
    coh           |sum_n U_n X_n| / sum_n |X_n|,  0 where the denominator is 0

model(..., truth=False) is the float32 composition in the kernels' order: the products, the sums over n per pixel in increasing
n from 0, one division.  (The alignment sum alone is taken in numpy's order, not the kernel's strided partials, butterfly and
waves: any order lies within tol_C below.)  model(..., truth=True) is everything in double from the definitions.  brute() is the
definitions as plain loops per group, repeat and A-scan, the check of both.

The tolerance, u = 2^-24, first order in u, from the truth alone.  M = sum_n |X_n|, S = sum_n U_n X_n.
  U             a complex float product is within 4 u |a| |b| of the exact one.  C is a float sum of k such products (k = count, or
                count x ascans with align 2), within tol_C = (k + 4) u sum |X_n| |X_ref| (Higham 4.2), which turns the unit phasor by
                turn = tol_C / |C| (first order); the phasor's own arithmetic -- hypotf, granted OpenCL's bound of 4 ulp = 8 u, and
                two divisions -- 12 u more.  A C that is exactly 0 -- a row or frame of zeros -- is exactly 0 on both sides: no turn.
  S             the turn U_n X_n is another complex product, 4 u: term n is within |X_n| (turn_n + 16 u), and the sum of N terms
                adds N u M:
                    e_S = sum_n |X_n| (turn_n + 16 u) + N u M          (turn_ref = 0, and every turn is 0 with align 0)
  mean          one division:  tol_mean = e_S / N + u |Z|, of the complex difference's modulus
  mag           hypotf, 8 u:   tol_mag = tol_mean + 8 u |Z|
  incoh         |X_n| is a square root of two products and a sum, 2.5 u; N positive terms, one division:
                    tol_incoh = (N + 4) u incoh
  coh           |S| within e_S + 8 u |S|, M within (N + 2.5) u M, the division:
                    tol_coh = e_S / M + (N + 12) u coh
Every tolerance is of the float value stored: there is no further rounding.

The adjudication is the project's own: |gpu - truth| / tol <= max(helpers.TRUTH_LIMIT, the float composition's own ratio), every
figure printed first and appended to helpers.TRUTH_LOG.

No pixel is exempt.  Instead the catalogue (tests/cxavg_cases.py) is held to a conditioning rule, which tests/test_cxavg_cases.py
asserts: for every (group, repeat, A-scan) of every case the truth's |C| is exactly 0 or at least 16 tol_C (tolerances()["condition"] is the smallest ratio)."""
import os

import numpy as np

import helpers

U = 2.0 ** -24
NAMES = ("mean", "mag", "incoh", "coh")
BLOCK, BLOCKS_PER_CU, REG_PAIRS = 256, 4, 16          # kCxaBlock, kCxaWavesPerCu / 4, kCxaRegPairs (fdoct_cxavg_kernels.h)
FORM_REGISTER, FORM_STREAMING = 1, 2
PLAN_CUS = 256                                        # what fdoct_cxavg_plan, which has no handle, takes for the card
CONDITION = 16.0
RATIOS = []   # (what, {output: (gpu ratio, f32 ratio)}), one per check()


def resolve_range(align, rng, depths):
    """(first, count) of the alignment sum, or None with align 0: count 0 means the rest."""
    if not align:
        return None
    first, cnt = rng
    return first, cnt if cnt else depths - first


def register_slots(repeats, depths):
    """cxavg_register_slots: the repeats rounded up to 2, 4, 8 or 16 where that many rows of ceil(depths / 256) pairs a thread fit
    REG_PAIRS, else 0 (the streaming form)."""
    nr = 2
    while nr < repeats:
        nr *= 2
    return nr if nr <= REG_PAIRS and nr * (-(-depths // BLOCK)) <= REG_PAIRS else 0


def geometry(nframes, repeats, stride, ascans, depths, align, cus=PLAN_CUS):
    """(groups, form, workgroups, workspace_bytes) of plan_cxavg and cxavg_plan_launch."""
    stride = repeats if stride is None else stride
    groups = (nframes - repeats) // stride + 1
    form = FORM_REGISTER if register_slots(repeats, depths) else FORM_STREAMING
    ws = (groups * repeats * (1 + ascans)) * 8 if align == 2 else 0
    return groups, form, min(groups * ascans, cus * BLOCKS_PER_CU), ws


def grouped(X, repeats, stride=None):
    """X (nframes, H, D) -> (G, N, H, D): group g's repeat n is frame g stride + n."""
    X = np.asarray(X)
    stride = repeats if stride is None else stride
    assert X.ndim == 3 and repeats >= 2 and 1 <= stride <= repeats and X.shape[0] >= repeats and (X.shape[0] - repeats) % stride == 0
    G = (X.shape[0] - repeats) // stride + 1
    return X[np.arange(G)[:, None] * stride + np.arange(repeats)[None, :]]


def _phasors(xr, xi, ref, align, rng, f):
    """(ux, uy) in type f, broadcastable to (G, N, H, D), and C (complex, (G, N, H) or (G, N)) -- None with align 0."""
    G, N = xr.shape[:2]
    if not rng:
        return np.ones((G, N, 1, 1), f), np.zeros((G, N, 1, 1), f), None
    s = slice(rng[0], rng[0] + rng[1])
    ar, ai, br, bi = xr[..., s], xi[..., s], xr[:, ref:ref + 1, :, s], xi[:, ref:ref + 1, :, s]
    axes = -1 if align == 1 else (-2, -1)
    Cr = (ar * br + ai * bi).sum(axes, dtype=f)
    Ci = (ai * br - ar * bi).sum(axes, dtype=f)
    m = np.hypot(Cr, Ci).astype(f)
    ok = m > 0
    ux = np.where(ok, Cr / np.where(ok, m, 1), 1).astype(f)
    uy = np.where(ok, -(Ci / np.where(ok, m, 1)), 0).astype(f)
    ux[:, ref], uy[:, ref] = 1, 0
    shape = (G, N, -1, 1) if align == 1 else (G, N, 1, 1)
    return ux.reshape(shape), uy.reshape(shape), Cr + 1j * Ci


def _compose(Xg, ref, align, rng, f):
    G, N, H, D = Xg.shape
    xr, xi = Xg.real.astype(f), Xg.imag.astype(f)
    ux, uy, C = _phasors(xr, xi, ref, align, rng, f)
    ux, uy = np.broadcast_to(ux, (G, N, H, 1)), np.broadcast_to(uy, (G, N, H, 1))
    zr, zi, m = np.zeros((G, H, D), f), np.zeros((G, H, D), f), np.zeros((G, H, D), f)
    for n in range(N):
        zr = zr + (xr[:, n] * ux[:, n] - xi[:, n] * uy[:, n])
        zi = zi + (xr[:, n] * uy[:, n] + xi[:, n] * ux[:, n])
        m = m + np.sqrt(xr[:, n] * xr[:, n] + xi[:, n] * xi[:, n])
    mr, mi = zr / f(N), zi / f(N)
    zero = m == 0
    out = dict(mean=(mr + 1j * mi).astype(np.complex64 if f == np.float32 else np.complex128), mag=np.hypot(mr, mi).astype(f), incoh=m / f(N),
               coh=np.where(zero, f(0), np.hypot(zr, zi).astype(f) / np.where(zero, f(1), m)).astype(f))
    assert all(out[k].dtype == f for k in NAMES[1:])
    return out, dict(C=C, S=zr + 1j * zi, M=m)


def model(X, repeats, stride=None, ref=0, align=1, align_range=(0, 0), truth=False):
    """dict(mean, mag, incoh, coh), each (groups, H, D): complex64 / float32, or complex128 / float64 with truth (which also returns
    C, S and M)."""
    Xg = grouped(X, repeats, stride)
    rng = resolve_range(align, align_range, Xg.shape[3])
    if truth:
        out, extra = _compose(np.asarray(Xg, np.complex128), ref, align, rng, np.float64)
        out.update(extra)
        return out
    return _compose(Xg, ref, align, rng, np.float32)[0]


def brute(X, repeats, stride=None, ref=0, align=1, align_range=(0, 0)):
    """The four outputs by the definitions, as plain loops in double."""
    Xg = np.asarray(grouped(X, repeats, stride), np.complex128)
    G, N, H, D = Xg.shape
    rng = resolve_range(align, align_range, D)
    out = dict(mean=np.zeros((G, H, D), np.complex128), mag=np.zeros((G, H, D)), incoh=np.zeros((G, H, D)), coh=np.zeros((G, H, D)))
    for g in range(G):
        for r in range(H):
            S, M = np.zeros(D, np.complex128), np.zeros(D)
            for n in range(N):
                u = 1.0
                if rng and n != ref:
                    rows = [r] if align == 1 else range(H)
                    C = sum(np.vdot(Xg[g, ref, q, rng[0]:rng[0] + rng[1]], Xg[g, n, q, rng[0]:rng[0] + rng[1]]) for q in rows)   # sum X_n conj(X_ref)
                    u = np.conj(C) / abs(C) if abs(C) > 0 else 1.0
                S = S + u * Xg[g, n, r]
                M = M + np.abs(Xg[g, n, r])
            out["mean"][g, r], out["mag"][g, r], out["incoh"][g, r] = S / N, np.abs(S / N), M / N
            out["coh"][g, r] = np.where(M == 0, 0.0, np.abs(S) / np.where(M == 0, 1.0, M))
    return out


def _turns(Xg, ref, align, rng, tr):
    """(tol_C, |C|, turn) per (G, N, H) or (G, N): the turn is 0 where tol_C is 0 (zeros), for the ref, and with align 0."""
    G, N, H, D = Xg.shape
    if not rng:
        z = np.zeros((G, N))
        return z, z, z
    s = slice(rng[0], rng[0] + rng[1])
    mag = np.abs(Xg[..., s]) * np.abs(Xg[:, ref:ref + 1, :, s])
    k = rng[1] * (H if align == 2 else 1)
    tol_C = (k + 4) * U * mag.sum(-1 if align == 1 else (-2, -1))
    absC = np.abs(tr["C"])
    live = tol_C > 0
    live[:, ref] = False
    turn = np.where(live, tol_C / np.where(live, np.maximum(absC, 1e-300), 1), 0.0)
    return np.where(live, tol_C, 0.0), np.where(live, absC, 0.0), turn


def tolerances(X, repeats, stride=None, ref=0, align=1, align_range=(0, 0)):
    """dict(mean, mag, incoh, coh (groups, H, D), truth, condition) from the truth alone.  condition: the smallest |C| / tol_C over
    the (group, repeat, A-scan) whose tol_C is not 0 (inf where there is none)."""
    Xg = np.asarray(grouped(X, repeats, stride), np.complex128)
    G, N, H, D = Xg.shape
    rng = resolve_range(align, align_range, D)
    tr = model(X, repeats, stride, ref, align, align_range, truth=True)
    tol_C, absC, turn = _turns(Xg, ref, align, rng, tr)
    turn4 = turn.reshape((G, N, -1, 1) if turn.ndim == 3 else (G, N, 1, 1))
    A = np.abs(Xg)
    M = A.sum(1)
    e_S = (A * (turn4 + 16 * U)).sum(1) + N * U * M
    Z = np.abs(tr["mean"])
    safe = np.where(M == 0, 1.0, M)
    tol_mean = e_S / N + U * Z
    live = tol_C > 0
    return dict(truth=tr, mean=tol_mean, mag=tol_mean + 8 * U * Z, incoh=(N + 4) * U * tr["incoh"], coh=e_S / safe + (N + 12) * U * tr["coh"],
                condition=float((absC[live] / tol_C[live]).min()) if live.any() else float("inf"))


def _ratio(got, ref, tol):
    """Worst |got - ref| / tol; a pixel whose tolerance is 0 must be exact."""
    err = np.abs(np.asarray(got).astype(np.complex128 if np.iscomplexobj(got) else np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rat = np.where(err == 0, 0.0, err / tol)
    return float(rat.max())


def check(gpu, X, what, refs=None, **kw):
    """gpu: dict of any of mean, mag, incoh, coh as the library wrote them.  Every output against the truth by the adjudication,
    every figure printed before anything is asserted.  refs: (model, tolerances) where the caller has them already."""
    if refs is None:
        refs = (model(X, **kw), tolerances(X, **kw))
    f32, tol = refs
    tr = tol["truth"]
    assert tol["condition"] >= CONDITION, "%s: |C| / tol_C = %.3g: the case is outside the conditioning rule" % (what, tol["condition"])
    names = [k for k in NAMES if k in gpu and gpu[k] is not None]
    for k in names:
        g = np.asarray(gpu[k])
        assert g.dtype == (np.complex64 if k == "mean" else np.float32) and g.shape == tr[k].shape, (what, k, g.dtype, g.shape)
        assert np.isfinite(g).all(), what + ": %s is not finite (an output pixel was not written)" % k
    figs = {k: (_ratio(gpu[k], tr[k], tol[k]), _ratio(f32[k], tr[k], tol[k])) for k in names}
    print("%s: |gpu - truth| / tol (f32 model) %s; |C| / tol_C >= %.3g" % (
        what, ", ".join("%s %.4f (%.4f)" % (k, figs[k][0], figs[k][1]) for k in names), tol["condition"]))
    RATIOS.append((what, figs))
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    for k in names:
        helpers.TRUTH_LOG.append((test, "%s (cxavg %s)" % (what, k), figs[k][0], figs[k][1]))
    for k in names:
        g, o = figs[k]
        assert g <= max(helpers.TRUTH_LIMIT, o), "%s: %s |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 model's own %.3g)" % (
            what, k, g, helpers.TRUTH_LIMIT, o)
    return figs
