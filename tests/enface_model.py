"""The quantity of include/fdoct_enface.h restated in numpy: the float32 model with the header's orders bit for bit, a float64
truth for the mean, and the derived tolerance between the two.  Parameters are the keywords of fdoct_amd.enface.params, as a dict:
slabs [(first, count)], surface (None, "absolute", "relative"), search (first, count), smooth, threshold, median.

The orders.  A candidate's box sum B[b] adds S[b + j] in increasing j from scratch.  A slab's sum is made of 64 partials, partial l
summing from 0, in increasing b, the slab's depths with (b mod 256) // 4 == l; then p[l] += p[l + k] for k = 32, 16, 8, 4, 2, 1 and
p[0] is the sum.  The mean is that sum divided by float32(n).  Max, argmax and the surface are exact: no tolerance.

The tolerance of the mean against the truth, for any summation order: n - 1 additions and one division, each with a relative error
of at most 2^-24, bound |mean - truth| by n 2^-24 mean|V| over the slab to first order; the second-order terms stay below 1 % of that
for n <= 2^16, hence 1.01 n 2^-24 mean|V|."""
import numpy as np

F = np.float32
SURFACES = {None: 0, "none": 0, "absolute": 1, "relative": 2, 0: 0, 1: 1, 2: 2}
DEFAULTS = dict(slabs=((0, 1),), surface=None, search=(0, 0), smooth=1, threshold=0.0, median=1)


def resolve(p, depths):
    """The parameters with their defaults, the surface as a number and the search range as [s0, s1)."""
    q = dict(DEFAULTS, **p)
    q["surface"] = SURFACES[q["surface"]]
    s0, cnt = q["search"]
    q["s0"], q["s1"] = s0, s0 + (cnt if cnt else depths - s0)
    return q


def box_sums(S, s0, s1, smooth):
    """B[..., i] for the candidates s0 + i, i <= s1 - smooth - s0, of every A-scan of S (float32)."""
    n = s1 - smooth - s0 + 1
    B = S[..., s0:s0 + n].copy()
    for j in range(1, smooth):
        B = B + S[..., s0 + j:s0 + j + n]
    assert B.dtype == F
    return B


def raw_surface(S, q):
    """z0: the smallest candidate whose box sum reaches the threshold, -1 where none does."""
    B = box_sums(S, q["s0"], q["s1"], q["smooth"])
    if q["surface"] == 1:
        thr = np.full(B.shape[:-1] + (1,), F(q["threshold"]) * F(q["smooth"]), F)
    else:
        with np.errstate(invalid="ignore"):
            m = np.max(np.where(np.isnan(B), F(-np.inf), B), axis=-1, keepdims=True)   # from -inf, replaced on B > m: NaN never enters
            thr = F(q["threshold"]) * m
    with np.errstate(invalid="ignore"):
        hit = B >= thr
    return np.where(hit.any(axis=-1), q["s0"] + np.argmax(hit, axis=-1), -1).astype(np.int32)


def lateral_median(z0, median):
    """The lower median of the valid raw surfaces within (median - 1) / 2 A-scans, per position."""
    P, H = z0.shape
    half = (median - 1) // 2
    z = np.full((P, H), -1, np.int32)
    for p in range(P):
        for r in range(H):
            w = z0[p, max(r - half, 0):min(r + half, H - 1) + 1]
            w = np.sort(w[w >= 0])
            if w.size:
                z[p, r] = w[(w.size - 1) // 2]
    return z


def slab_bounds(z, first, count, depths):
    """The clipped slab [lo, hi) of every A-scan; hi <= lo where nothing remains (z = -1 included)."""
    lo = np.maximum(z.astype(np.int64) + first, 0)
    hi = np.minimum(z.astype(np.int64) + first + count, depths)
    hi = np.where(z < 0, lo, hi)
    return lo, np.maximum(hi, lo)


def slab_sums(V, lo, hi):
    """The header's order, bit for bit: V (rows, depths) float32, lo / hi per row."""
    R, D = V.shape
    p = np.zeros((R, 64), F)
    if R == 0 or not np.any(hi > lo):
        return p[:, 0]
    lanes = np.arange(64)
    for c in range(int(lo[hi > lo].min()) // 256 * 256, int(hi.max()), 256):
        for j in range(4):
            b = c + 4 * lanes + j
            inside = (b[None, :] >= lo[:, None]) & (b[None, :] < hi[:, None])
            x = V[:, np.minimum(b, D - 1)]
            p = np.where(inside, p + x, p)
    assert p.dtype == F
    k = 32
    while k >= 1:
        p[:, :k] = p[:, :k] + p[:, k:2 * k]
        k //= 2
    return p[:, 0]


def model(V, p, S=None):
    """Every output of fdoct_enface for the volume V (positions, ascans, depths) float32, and what the tests hold them to:
    mean / max / argmax (nslabs, positions, ascans), surface and z0 (positions, ascans; absent without a surface), n (the depths that
    remain of every slab), truth (the float64 mean) and bound (the tolerance of mean against truth)."""
    V = np.ascontiguousarray(V, F)
    P, H, D = V.shape
    q = resolve(p, D)
    out = {}
    if q["surface"]:
        out["z0"] = raw_surface(V if S is None else np.ascontiguousarray(S, F), q)
        z = out["surface"] = lateral_median(out["z0"], q["median"])
    else:
        z = np.zeros((P, H), np.int32)
    ns = len(q["slabs"])
    rows = V.reshape(P * H, D)
    depth = np.arange(D)
    for k, dt in (("mean", F), ("max", F), ("argmax", np.int32), ("n", np.int64), ("truth", np.float64), ("bound", np.float64)):
        out[k] = np.zeros((ns, P, H), dt)
    for s, (first, count) in enumerate(q["slabs"]):
        lo, hi = slab_bounds(z.reshape(-1), first, count, D)
        n = hi - lo
        some = n > 0
        inside = (depth[None, :] >= lo[:, None]) & (depth[None, :] < hi[:, None])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(some, slab_sums(rows, lo, hi) / n.astype(F), F(0)).astype(F)
            masked = np.where(inside, rows, F(-np.inf))
            am = np.argmax(masked, axis=1)               # the first maximum
            mx = masked[np.arange(P * H), am]
            truth = np.where(some, np.where(inside, rows, 0).astype(np.float64).sum(axis=1) / np.maximum(n, 1), 0.0)
            mean_abs = np.where(some, np.where(inside, np.abs(rows), 0).astype(np.float64).sum(axis=1) / np.maximum(n, 1), 0.0)
        out["mean"][s] = mean.reshape(P, H)
        out["max"][s] = np.where(some, mx, F(0)).reshape(P, H)
        out["argmax"][s] = np.where(some, am, -1).reshape(P, H)
        out["n"][s] = n.reshape(P, H)
        out["truth"][s] = truth.reshape(P, H)
        out["bound"][s] = (1.01 * n * 2.0 ** -24 * mean_abs).reshape(P, H)
    return out


def brute(V, p, S=None):
    """The same quantity by plain loops over scalars, independent of the above in everything but the definitions: the integer outputs
    and the maximum exactly, the mean in float64 (held to `bound`, not to bits)."""
    V = np.asarray(V, F)
    S = V if S is None else np.asarray(S, F)
    P, H, D = V.shape
    q = resolve(p, D)
    ns = len(q["slabs"])
    z0 = np.full((P, H), -1, np.int32)
    if q["surface"]:
        for pp in range(P):
            for r in range(H):
                Bs = []
                for b in range(q["s0"], q["s1"] - q["smooth"] + 1):
                    acc = S[pp, r, b]
                    for j in range(1, q["smooth"]):
                        acc = F(acc + S[pp, r, b + j])
                    Bs.append(acc)
                if q["surface"] == 1:
                    thr = F(F(q["threshold"]) * F(q["smooth"]))
                else:
                    m = F(-np.inf)
                    for B in Bs:
                        if B > m:
                            m = B
                    thr = F(F(q["threshold"]) * m)
                for i, B in enumerate(Bs):
                    if B >= thr:
                        z0[pp, r] = q["s0"] + i
                        break
    out = dict(mean=np.zeros((ns, P, H)), max=np.zeros((ns, P, H), F), argmax=np.full((ns, P, H), -1, np.int32))
    z = np.zeros((P, H), np.int32)
    if q["surface"]:
        half = (q["median"] - 1) // 2
        for pp in range(P):
            for r in range(H):
                vals = sorted(int(z0[pp, rr]) for rr in range(r - half, r + half + 1) if 0 <= rr < H and z0[pp, rr] >= 0)
                z[pp, r] = vals[(len(vals) - 1) // 2] if vals else -1
        out["z0"], out["surface"] = z0, z
    for s, (first, count) in enumerate(q["slabs"]):
        for pp in range(P):
            for r in range(H):
                if z[pp, r] < 0:
                    continue
                lo, hi = max(z[pp, r] + first, 0), min(z[pp, r] + first + count, D)
                if hi <= lo:
                    continue
                acc, m, a = 0.0, V[pp, r, lo], lo
                for b in range(lo, hi):
                    acc += float(V[pp, r, b])
                    if V[pp, r, b] > m:
                        m, a = V[pp, r, b], b
                out["mean"][s, pp, r], out["max"][s, pp, r], out["argmax"][s, pp, r] = acc / (hi - lo), m, a
    return out
