"""CPU tests of tests/lowpass_model.py, the numpy restatement of BscanDark's lpfilter (BscanDark.cpp:119-167): the literal
steps against the closed form the kernel of fdoct_lowpass.hip evaluates, and the properties a low-pass projector has.  Every
bound is 1e-12 of the row's largest sample: float64 sums of at most 2048 terms of that size round at 1e-16 each."""
import numpy as np
import pytest

import lowpass_model
from lowpass_model import lowpass_closed_form, lpfilter_f32, lpfilter_truth

WIDTHS = [2, 7, 9, 10, 11, 19, 20, 21, 128, 129, 640, 1280, 2048]
BOUND = 1e-12


def _rows(W, seed=1, n=3):
    return np.random.default_rng(seed + W).uniform(0.0001, 1.0, (n, W))


def _close(a, b, scale):
    assert np.abs(a - b).max() <= BOUND * scale, np.abs(a - b).max() / scale


@pytest.mark.parametrize("W", WIDTHS)
def test_literal_steps_equal_the_closed_form(W):
    x = _rows(W)
    _close(lpfilter_truth(x), lowpass_closed_form(x), x.max())
    x = x * 16 * 65535.0     # raw sums of 16 frames
    _close(lpfilter_truth(x), lowpass_closed_form(x), x.max())


@pytest.mark.parametrize("W", [2, 3, 7, 8, 9])
def test_widths_below_ten_give_zeros(W):
    x = _rows(W)
    assert np.all(lpfilter_truth(x) == 0.0) and np.all(lpfilter_f32(x) == 0.0) and np.all(lowpass_closed_form(x) == 0.0)


def test_a_single_column_blanks_nothing():
    """W = 1: cx = dcl = dcr = 0, so steps 3-5 touch nothing and the one-point transforms return the sample."""
    x = _rows(1)
    assert np.array_equal(lpfilter_truth(x), x) and np.array_equal(lowpass_closed_form(x), x)
    assert np.array_equal(lpfilter_f32(x), x.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("W", [w for w in WIDTHS if w >= 20])
def test_filter_is_a_projector(W):
    x = _rows(W)
    y = lpfilter_truth(x)
    _close(lpfilter_truth(y), y, x.max())                 # idempotent: an off-by-one in dcl / dcr would not be
    c = np.full((1, W), 0.375)
    _close(lpfilter_truth(c), c, 0.375)                   # a constant row passes
    f = W // 10
    n = np.arange(W)
    for phase in (0.0, 0.7):
        kept = np.cos(2 * np.pi * (f - 1) * n / W + phase)[None]
        gone = np.cos(2 * np.pi * f * n / W + phase)[None]
        _close(lpfilter_truth(kept), kept, 1.0)           # the last kept bin
        _close(lpfilter_truth(gone), np.zeros((1, W)), 1.0)   # the first blanked one


def test_f32_restatement_stays_far_inside_the_tolerance():
    """The allowance of the GPU tests is max(0.5, f32 model's own distance): on inputs like theirs that distance is small, so
    0.5 x tol is the bound that binds."""
    rng = np.random.default_rng(3)
    for x in (rng.uniform(0.0001, 1.0, (8, 2048)), rng.uniform(0, 16 * 65535.0, (8, 2048)), rng.uniform(0.0001, 1.0, (4, 129))):
        t = lpfilter_truth(x)
        assert (np.abs(lpfilter_f32(x) - t) / lowpass_model.tolerance(t)).max() < 0.25
        worst, excess = lowpass_model.parity(lowpass_closed_form(x), x)
        assert worst < 1e-6 and excess < 0


def test_parity_rule_rejects_a_wrong_band():
    x = _rows(640)
    n = np.arange(640)
    wrong = lpfilter_truth(x) + 1e-3 * np.cos(2 * np.pi * 64 * n / 640)[None]   # one bin too many
    assert lowpass_model.parity(wrong, x)[1] > 0
    assert lowpass_model.parity(np.full((1, 7), 1e-30), _rows(7, n=1))[1] > 0     # W < 10 must be exact zeros
