"""The fields and cases of the dispersion search's tests (tests/test_dispersion_cases.py on the CPU, tests/test_gpu_dispersion.py on
the card), held to tests/dispersion_model.py.

The field.  z[r][q] = hann[q] sum_k a_k cos(2 pi d_k q / n + phi(q; a2*, a3*)) + 0.02 N(0, 1) (seeded): three reflectors (d, a) =
(0.11 n + 1.7 r, 1.0), (0.23 n + 0.9 r, 0.6), (0.36 n - 0.5 r, 0.35) seen through the planted dispersion (a2*, a3*), and
X = n ifft(z) as complex64: the complex A-scans a chain without a phase would give.  The search's candidate (a2*, a3*) undoes the
phase on the positive depths, so a grid that holds the planted pair should find it.

The grid is a2 in -24 .. 24 step 4 and a3 in -8 .. 8 step 2 (K = 117: 15 chunks of 8 candidates, the last of 5 -- fdoct_dispersion_plan's
own figures, asserted by the tests) over bins [2, n/2), except where a case says otherwise.  Sizes: the smallest at which the planted
pair is recovered with a clear margin (64 x 2 is too small: not recovered), lengths with factors 3 and 5, and one of 4096, the
longest the stage takes, whose margin is clear but whose winner is a neighbour of the planted pair (not a recovery case)."""
import numpy as np

import dispersion_model as dm

A2, A3 = (-24.0, 4.0, 13), (-8.0, 2.0, 9)
REFLECTORS = ((0.11, 1.7, 1.0), (0.23, 0.9, 0.6), (0.36, -0.5, 0.35))


def field(n, rows, planted, seed, zero_row=None):
    """X (rows, n) complex64."""
    rng = np.random.default_rng(seed)
    q = np.arange(n, dtype=np.float64)
    x = dm.x_of(n)
    phi = planted[0] * x ** 2 + planted[1] * x ** 3
    z = np.zeros((rows, n))
    for r in range(rows):
        for d, slope, amp in REFLECTORS:
            z[r] += amp * np.cos(2 * np.pi * (d * n + slope * r) * q / n + phi)
        z[r] *= np.hanning(n)
    z += 0.02 * rng.standard_normal((rows, n))
    X = (n * np.fft.ifft(z, axis=-1)).astype(np.complex64)
    if zero_row is not None:
        X[zero_row] = 0
    return X


def _case(what, n, rows, planted, a2=A2, a3=A3, depth=None, recovery=False, zero_row=None, brute=True):
    return dict(what=what, n=n, rows=rows, planted=planted, a2=a2, a3=a3, depth=depth if depth is not None else (2, n // 2 - 2), recovery=recovery,
                zero_row=zero_row, brute=brute)


CASES = [
    _case("96x3 planted (8,-2)", 96, 3, (8.0, -2.0), recovery=True),
    _case("128x4 planted (12,-4)", 128, 4, (12.0, -4.0), recovery=True),
    _case("160x3 planted (-20,6)", 160, 3, (-20.0, 6.0), recovery=True),
    _case("192x2 planted (4,4)", 192, 2, (4.0, 4.0), recovery=True),
    _case("4096x1 planted (12,-4)", 4096, 1, (12.0, -4.0), brute=False),
    _case("96x2 one candidate", 96, 2, (8.0, -2.0), a2=(8.0, 4.0, 1), a3=(-2.0, 2.0, 1)),
    _case("128x2 a2 alone", 128, 2, (12.0, -4.0), a3=(-4.0, 2.0, 1)),
    # (every bin of a real spectrum's A-scan: candidates (a2, a3) and (-a2, -a3) tie by symmetry, so the grid holds a2 > 0 only)
    _case("96x2 every bin", 96, 2, (8.0, -2.0), a2=(4.0, 4.0, 6), depth=(0, 96)),
    # (one bin holds little to tell candidates apart: a coarser grid, 25 candidates, at the bin where the model's margin is clear)
    _case("128x3 one bin", 128, 3, (12.0, -4.0), a2=(-24.0, 12.0, 5), a3=(-8.0, 4.0, 5), depth=(15, 1)),
    _case("128x4 a zero row", 128, 4, (12.0, -4.0), zero_row=2),
    _case("160x2 default range", 160, 2, (-20.0, 6.0), depth=(0, 0)),
]

_FIELDS, _MODELS = {}, {}


def case_field(case):
    """The case's X, made once and handed out read-only."""
    k = case["what"]
    if k not in _FIELDS:
        X = field(case["n"], case["rows"], case["planted"], seed=1000 + CASES.index(case), zero_row=case["zero_row"])
        X.setflags(write=False)
        _FIELDS[k] = X
    return _FIELDS[k]


def case_models(case):
    """(truth, float composition) of the case, computed once."""
    k = case["what"]
    if k not in _MODELS:
        X = case_field(case)
        _MODELS[k] = (dm.model(X, case["a2"], case["a3"], case["depth"], truth=True), dm.model(X, case["a2"], case["a3"], case["depth"], truth=False))
    return _MODELS[k]


def planted_index(case):
    v2, v3 = dm.axis_values(*case["a2"]), dm.axis_values(*case["a3"])
    i2, i3 = int(np.argmin(np.abs(v2 - case["planted"][0]))), int(np.argmin(np.abs(v3 - case["planted"][1])))
    return i2 * len(v3) + i3
