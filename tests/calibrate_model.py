"""The specification of include/fdoct_calibrate.h in numpy: BscanDark's three captures and their composition
data_yb = (data_yr - data_yd) + (data_ys - data_yd) (BscanDark.cpp:996, 1005-1222), built on tests/capture_model.py (the key
handlers' recipe) and tests/lowpass_model.py (lpfilter).  What those two state is imported, not restated; this module adds the
composition, cv::normalize(NORM_MINMAX) per row or per plane as one function, and the input planes of the tests with the
conditions each is chosen for."""
from fractions import Fraction

import numpy as np

import capture_model
import lowpass_model
import oracle_lib
from capture_model import bits  # noqa: F401  (the tests compare doubles as words)

DARK, REFERENCE, SAMPLE = range(3)            # fdoct_cal_slot
CAPTURE_LIMITS = (0.0001, 1.0)                # BscanDark.cpp:1056-1061
EPS = float(np.finfo(np.float64).eps)         # DBL_EPSILON


def normalize_rows_minmax(y, lo, hi, per_row):
    """cv::normalize(.., lo, hi, NORM_MINMAX) on a (rows, width) float64 array: every row on its own (normalizerows,
    BscanDark.cpp:82-90) or the whole plane."""
    y = np.ascontiguousarray(y, np.float64)
    assert y.ndim == 2
    if per_row:
        return oracle_lib.normalizerows(y, lo, hi)
    return oracle_lib.normalize_minmax(y.ravel(), lo, hi).reshape(y.shape)


def capture(frames, lowpass=False, **recipe):
    """What a slot holds after fdoct_calibrate_capture saw `frames`: the recipe of the accumulating roles (capture_model.capture
    with role NONE; `recipe` are its keywords), then lpfilter in double if the lowpass option is set."""
    y = capture_model.capture(capture_model.NONE, frames, **recipe)
    return lowpass_model.lpfilter_truth(y) if lowpass else y


def compose(yr, ys, yd):
    """BscanDark.cpp:996 on float64 arrays, each operation rounded on its own."""
    yr, ys, yd = (np.asarray(a, np.float64) for a in (yr, ys, yd))
    return (yr - yd) + (ys - yd)


def host_loop(yr, ys, yd):
    """The loop a host runs today: for i: yr[i] = (yr[i] - yd[i]) + (ys[i] - yd[i]), on Python floats."""
    shape = np.shape(yr)
    r, s, d = (np.asarray(a, np.float64).ravel().tolist() for a in (yr, ys, yd))
    return np.array([(r[i] - d[i]) + (s[i] - d[i]) for i in range(len(r))], np.float64).reshape(shape)


# ---- the arithmetic of one normalisation, element by element ----------------------------------------------------------------
def coefficients(smin, smax, lo, hi):
    """(scale, shift) as fdoct_normalize_minmax forms them, every operation rounded on its own (Python floats are doubles)."""
    dmin, dmax = (lo, hi) if lo < hi else (hi, lo)
    scale = (dmax - dmin) * (1.0 / (smax - smin) if smax - smin > EPS else 0.0)
    return scale, dmin - smin * scale


def separate(y, scale, shift):
    """y * scale + shift, the product rounded before the sum."""
    prod = float(y) * scale
    return prod + shift


def fused(y, scale, shift):
    """What a fused multiply-add gives: the exact y * scale + shift rounded once (math.fma where Python has it, otherwise exact
    rational arithmetic; float(Fraction) rounds to nearest even)."""
    import math
    if hasattr(math, "fma"):
        return math.fma(float(y), scale, shift)
    return float(Fraction(float(y)) * Fraction(scale) + Fraction(shift))


# ---- input planes and what each is chosen for -----------------------------------------------------------------------------------
def plane(rows, width, seed):
    """Accumulated camera counts with noise: positive doubles that are no integers, a different range in every row."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(2e3, 6e4, (rows, 1))
    return level * rng.uniform(0.2, 1.0, (rows, width)) + rng.random((rows, width))


def no_contraction_plane():
    """5 x 24 doubles on which a fused y * scale + shift and the separately rounded one differ in some element, per row and per
    plane (tests/test_calibrate_model.py checks that they do)."""
    return plane(5, 24, seed=996)


def constant_row_plane():
    """3 x 8: row 1 is constant, so max - min <= DBL_EPSILON there and per-row normalisation gives `shift` = min(lo, hi) in every
    element of it; the other rows are ordinary."""
    y = plane(3, 8, seed=82)
    y[1, :] = 1234.5
    return y


def extremes_plane(rows, width, seed, min_at, max_at):
    """A plane whose only minimum and only maximum are at the (row, column) positions given: every other sample lies strictly
    between them."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(1000.0, 2000.0, (rows, width))
    y[min_at] = 3.25
    y[max_at] = 70000.5
    return y


def rows_extremes_plane(rows, width, seed):
    """A plane every row of which has its only minimum in its last column and its only maximum two columns before (width >= 3),
    with different values in every row."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(1000.0, 2000.0, (rows, width))
    r = np.arange(rows, dtype=np.float64)
    y[:, width - 1] = 3.25 + r / 1024.0
    y[:, width - 3] = 70000.5 - r / 1024.0
    return y
