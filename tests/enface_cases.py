"""The catalogue of the en-face stage's GPU cases (tests/test_gpu_enface.py runs every one against tests/enface_model.py;
tests/test_enface_cases.py holds each to the condition its name promises, on the model alone).  A case is a name, a volume (and
perhaps a structure volume) and the parameters as the keywords of fdoct_amd.enface.params.  Shapes are the smallest at which the
kernels can still go wrong: depths 1, 3, 67, 130, 257 (no multiple of 4 or 64, more than one block of 256), ascans 1, 3, 70 (more
than one wavefront's workgroup, a median window inside and at the edges), positions 1 .. 3.  No case exempts a pixel."""
import numpy as np

F = np.float32


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _noise(name, shape, lo=0.0, hi=1.0):
    return _rng(name).uniform(lo, hi, shape).astype(F)


def _steps(name, P, H, D, z, low=0.05, high=1.0):
    """Noise below `low` in front of depth z[p][r] and `high` plus noise from it on; z < 0: noise only."""
    V = _noise(name, (P, H, D), 0.0, low)
    for p in range(P):
        for r in range(H):
            if z[p][r] >= 0:
                V[p, r, z[p][r]:] += F(high)
    return V


def _fixed():
    return dict(V=_rng("fixed").normal(0, 1, (2, 3, 67)).astype(F), p=dict(slabs=[(0, 67), (5, 1), (60, 7), (66, 9)]))


def _ties():
    # small integers: every slab's maximum occurs several times, in one lane's four depths, across lanes and across blocks
    return dict(V=_rng("ties").integers(0, 4, (1, 3, 130)).astype(F), p=dict(slabs=[(0, 130), (10, 70), (3, 2)]))


def _no_crossing():
    P, H, D = 2, 70, 67
    z = [[10 + (r * 7) % 40 for r in range(H)] for _ in range(P)]
    z[0][10] = -1                      # alone: its neighbours give it a surface
    for r in range(30, 46):
        z[0][r] = -1                   # a run longer than the window: 32 .. 43 find nothing within two A-scans
    z[1][0] = z[1][69] = -1            # at the edges
    return dict(V=_steps("no crossing", P, H, D, z), p=dict(slabs=[(-2, 5), (3, 20)], surface="absolute", threshold=0.5, smooth=3, median=5))


def _clipped():
    P, H, D = 3, 3, 130
    z = [[1, 60, 125], [125, 1, 60], [0, 129, 64]]
    return dict(V=_steps("clipped", P, H, D, z), p=dict(slabs=[(-5, 10), (0, 20), (-100, 10), (100, 10), (-129, 1 << 30)], surface="absolute", threshold=0.5))


def _negative():
    # dB-like: everything below zero, so that a maximum started from 0 -- or an empty lane's 0 taken for a value -- shows
    return dict(V=_noise("negative", (1, 3, 257), -80.0, -40.0), p=dict(slabs=[(0, 257), (100, 64), (-3, 2)], surface="absolute", threshold=-55.0, smooth=4, median=3))


def _last_candidate():
    V = np.zeros((1, 3, 67), F)
    V[0, 0, 19:23] = 1                 # B[19] = 4 >= 3.6 > B[18] = 3: the last candidate of the search range [3, 23)
    V[0, 1, 8:30] = 1
    V[0, 2, 19:40] = 1                 # what lies beyond the range is not read
    return dict(V=V, p=dict(slabs=[(0, 4), (-3, 10)], surface="absolute", search=(3, 20), threshold=0.9, smooth=4))


def _relative():
    P, H, D = 2, 70, 257
    V = _noise("relative", (P, H, D), 0.0, 0.2)
    b = np.arange(D)
    for p in range(P):
        for r in range(H):
            V[p, r] += (2.0 * np.exp(-0.5 * ((b - (40 + 3 * (r % 50) + 20 * p)) / 6.0) ** 2)).astype(F)
    return dict(V=V, p=dict(slabs=[(0, 64), (-10, 20), (64, 64), (128, 200)], surface="relative", threshold=0.5, smooth=4, median=5))


def _one_depth():
    return dict(V=np.full((1, 1, 1), 2.5, F), p=dict(slabs=[(0, 1), (0, 5)], surface="absolute", threshold=2.5))


def _three_depths():
    V = np.array([[[1, 3, 2]], [[5, 5, 4]], [[-1, -2, -0.5]]], F)
    return dict(V=V, p=dict(slabs=[(0, 3), (-1, 2), (1, 1)], surface="relative", threshold=1.0))


def _wide_windows():
    # smooth 16 and median 15 over the 3 A-scans there are
    P, H, D = 2, 3, 130
    z = [[20, -1, 90], [50, 51, 49]]
    return dict(V=_steps("wide windows", P, H, D, z), p=dict(slabs=[(0, 30), (16, 1)], surface="relative", threshold=0.6, smooth=16, median=15))


def _structure():
    P, H, D = 1, 70, 67
    z = [[5 + (r * 11) % 50 for r in range(H)]]
    return dict(V=_rng("structure v").normal(0, 1, (P, H, D)).astype(F), S=_steps("structure", P, H, D, z),
                p=dict(slabs=[(0, 10), (-4, 8)], surface="absolute", threshold=0.5, smooth=2, median=3))


def _eight_slabs():
    slabs = [(0, 257), (0, 64), (64, 64), (128, 64), (192, 65), (255, 1), (250, 100), (3, 250)]
    return dict(V=_rng("eight slabs").normal(0, 1, (2, 3, 257)).astype(F), p=dict(slabs=slabs))


def _far_slabs():
    # slabs with blocks of 256 depths between them that nothing reads, behind a surface
    P, H, D = 1, 3, 1100
    z = [[4, 40, 300]]
    return dict(V=_steps("far slabs", P, H, D, z), p=dict(slabs=[(0, 3), (700, 90), (-4, 4)], surface="absolute", threshold=0.5, median=1))


_MAKERS = {"fixed": _fixed, "ties": _ties, "no crossing": _no_crossing, "clipped": _clipped, "negative": _negative, "last candidate": _last_candidate,
           "relative": _relative, "one depth": _one_depth, "three depths": _three_depths, "wide windows": _wide_windows, "structure": _structure,
           "eight slabs": _eight_slabs, "far slabs": _far_slabs}
NAMES = tuple(_MAKERS)


def case(name):
    """The case as a dict: name, V, S (None: the volume itself), p."""
    c = _MAKERS[name]()
    c.setdefault("S", None)
    c["name"] = name
    return c
