"""CPU checks of tests/calibrate_model.py and tests/calibrate_sizes.py: the model's normalisation equals the library's host helper
fdoct_normalize_minmax bit for bit, its composition equals the host loop of INTEGRATION.md 2d, and every input of
tests/test_gpu_calibrate.py meets the condition it is chosen for -- the no-contraction plane tells a fused multiply-add from two
roundings, the constant row has no range, and the planes beyond one grid pass place their extremes in the last stride."""
import numpy as np
import pytest

import calibrate_model as cm
import calibrate_sizes as cs
import capture_model
import lowpass_model
from calibrate_model import bits
from fdoct_amd import capi

CUS = [64, 104, 256, 304]
SHAPES = [(3, 8), (5, 24), (1, 1), (7, 161)]
LIMITS = [(0.0001, 1.0), (1.0, 0.0001), (-2.5, 17.0)]


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), what


def _planes():
    for rows, width in SHAPES:
        yield "%d x %d" % (rows, width), cm.plane(rows, width, seed=rows * 1000 + width)
    yield "constant row", cm.constant_row_plane()
    yield "no contraction", cm.no_contraction_plane()
    yield "negative and zero", np.array([[-3.0, 0.0, -0.0, 7.5], [1e-300, -1e-300, 0.0, 0.0]])


@pytest.mark.parametrize("lo,hi", LIMITS)
def test_model_equals_the_host_helper_bit_for_bit(lo, hi):
    for what, y in _planes():
        _same(cm.normalize_rows_minmax(y, lo, hi, False), capi.normalize_minmax(y.ravel(), lo, hi).reshape(y.shape), what + ", plane")
        _same(cm.normalize_rows_minmax(y, lo, hi, True), np.stack([capi.normalize_minmax(r, lo, hi) for r in y]), what + ", rows")
        # ... and element by element with the arithmetic the header states
        for per_row in (False, True):
            want = cm.normalize_rows_minmax(y, lo, hi, per_row)
            for r, row in enumerate(y):
                src = row if per_row else y
                scale, shift = cm.coefficients(float(src.min()), float(src.max()), lo, hi)
                _same(want[r], np.array([cm.separate(v, scale, shift) for v in row]), what)


def test_composition_equals_the_host_loop():
    yd, yr, ys = (cm.plane(6, 32, seed=s) for s in (1, 2, 3))
    _same(cm.compose(yr, ys, yd), cm.host_loop(yr, ys, yd))
    # the order of operations counts: another association of the same sum differs somewhere
    assert not np.array_equal(bits(cm.compose(yr, ys, yd)), bits((yr + ys) - 2.0 * yd))
    # ... and on captures as the library makes them (normalised to [0.0001, 1])
    f = np.random.default_rng(4).integers(0, 4096, (3, 2, 6, 32)).astype(np.uint16)
    cap = [cm.capture(x, rowwisenormalize=1, donotnormalize=0) for x in f]
    _same(cm.compose(cap[1], cap[2], cap[0]), cm.host_loop(cap[1], cap[2], cap[0]))


def test_model_capture_is_the_capture_models_recipe_and_the_lowpass_models_filter():
    f = np.random.default_rng(5).integers(0, 4096, (3, 6, 32)).astype(np.uint16)
    kw = dict(rowwisenormalize=1, donotnormalize=1, movavgn=2)
    plain = capture_model.capture(capture_model.NONE, f, **kw)
    _same(cm.capture(f, **kw), plain)
    _same(cm.capture(f, lowpass=True, **kw), lowpass_model.lpfilter_truth(plain))
    assert (cm.DARK, cm.REFERENCE, cm.SAMPLE) == (capi.CAL_DARK, capi.CAL_REFERENCE, capi.CAL_SAMPLE) == (0, 1, 2)


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("lo,hi", LIMITS[:2])
def test_no_contraction_plane_tells_a_fused_multiply_add_from_two_roundings(lo, hi, per_row):
    y = cm.no_contraction_plane()
    want = cm.normalize_rows_minmax(y, lo, hi, per_row)
    differ = 0
    for r, row in enumerate(y):
        src = row if per_row else y
        scale, shift = cm.coefficients(float(src.min()), float(src.max()), lo, hi)
        for c, v in enumerate(row):
            assert cm.separate(v, scale, shift) == want[r, c]
            differ += cm.fused(v, scale, shift) != want[r, c]
    assert differ >= 1, "a kernel that contracts y * scale + shift would pass on this plane"
    # the fused form is the exact value rounded once
    assert cm.fused(3.0, 1.0 / 3.0, -1.0) != 0.0 and cm.separate(3.0, 1.0 / 3.0, -1.0) == 0.0


@pytest.mark.parametrize("lo,hi", LIMITS)
def test_constant_row_has_no_range_and_yields_shift(lo, hi):
    y = cm.constant_row_plane()
    assert y[1].max() - y[1].min() <= cm.EPS and y[0].max() - y[0].min() > cm.EPS and y[2].max() - y[2].min() > cm.EPS
    scale, shift = cm.coefficients(float(y[1].min()), float(y[1].max()), lo, hi)
    assert scale == 0.0 and shift == min(lo, hi)
    got = cm.normalize_rows_minmax(y, lo, hi, True)
    assert np.all(got[1] == shift) and len(np.unique(got[0])) > 1


@pytest.mark.parametrize("cus", CUS)
def test_minmax_shape_invariants(cus):
    for rows, width in SHAPES + [cs.tall_thin(cus), cs.wide(cus), (1000, 2048), (1, 3), (1000, 1), (200000, 2)]:
        for per_row in (False, True):
            s = cs.minmax_shape(rows, width, per_row, cus)
            assert s["T"] in (1, 2, 4, 8, 16, 32, 64) and s["T2"] in (1, 2, 4, 8, 16, 32, 64) and 1 <= s["S"] <= cs.MAX_SEGMENTS
            assert s["T"] >= min(64, s["items"]) and s["T"] < 2 * max(1, min(64, s["items"]))   # no wider than the group has runs
            assert (s["S"] - 1) * s["T"] < s["items"]                       # no segment is empty
            assert s["units"] <= max(s["groups"], s["teams"])               # segments never push the units beyond one pass
            assert s["blocks"] <= cs.resident(cus) and s["blocks2"] <= cs.resident(cus)
            assert s["ws_doubles"] == 2 * s["groups"] * s["S"] + 2 * s["groups"]


@pytest.mark.parametrize("cus", CUS)
def test_tall_thin_plane_lies_beyond_one_pass(cus):
    H, W = cs.tall_thin(cus)
    assert W == 4 and W < 64
    rows = cs.minmax_shape(H, W, True, cus)
    assert rows["T"] == 2 and rows["S"] == 1 and rows["units"] == H                 # a team of two lanes a row
    assert cs.beyond(H, rows["teams"]) and rows["blocks"] == cs.resident(cus)       # more rows than the capped grid has teams
    assert rows["T2"] == 1 and rows["blocks2"] == cs.resident(cus) and cs.beyond(H, cs.lanes(cus))   # pass 2: one thread a row
    assert cs.beyond(2 * H, cs.lanes(cus))                                          # the scale pass
    assert H * W * 8 < 32 << 20
    # as one plane: the extremes lie in the last pass of their team's loop
    whole = cs.minmax_shape(H, W, False, cus)
    assert whole["items"] == 2 * H > whole["step"] and whole["T"] == 64
    min_at, max_at = cs.extreme_positions(H, W)
    last = cs.last_pass_start(whole["items"], whole["step"])
    assert last > 0 and cs.run_of(*min_at, W) >= last and cs.run_of(*max_at, W) >= last
    assert cs.run_of(*min_at, W) != cs.run_of(*max_at, W)
    # per row: the rows of the last pass exist, and every row's extremes are two different runs
    assert cs.last_pass_start(H, rows["teams"]) >= rows["teams"]
    y = cm.rows_extremes_plane(8, W, seed=1)
    assert np.all(y.argmin(axis=1) == W - 1) and np.all(y.argmax(axis=1) == W - 3) and len(set(y[:, W - 1])) == 8


@pytest.mark.parametrize("cus", CUS)
def test_wide_plane_lies_beyond_one_pass(cus):
    H, W = cs.wide(cus)
    assert H == 3 and W % 2 == 1 and (W * 8) % 16 != 0                             # packed rows alternate in 16-byte alignment
    cpr = -(-W // 2)
    assert cs.beyond(H * cpr, cs.lanes(cus)) and H * W * 8 < 32 << 20              # the scale pass
    min_at, max_at = cs.extreme_positions(H, W)
    for per_row in (False, True):
        s = cs.minmax_shape(H, W, per_row, cus)
        assert s["T"] == 64 and s["S"] > 64 and s["T2"] == 64                       # pass 2 strides over the partials too
        assert 2 * s["items"] >= 3 * s["step"]                                      # every lane loads in more than one pass
        last = cs.last_pass_start(s["items"], s["step"])
        group_run = (lambda at: cs.run_of(0, at[1], W)) if per_row else (lambda at: cs.run_of(*at, W))
        assert last > 0 and group_run(min_at) >= last and group_run(max_at) >= last
    y = cm.extremes_plane(H, 9, 2, *cs.extreme_positions(H, 9))
    assert np.unravel_index(y.argmin(), y.shape) == (H - 1, 8) and np.unravel_index(y.argmax(), y.shape) == (H - 1, 6)
    assert np.sum(y == y.min()) == 1 and np.sum(y == y.max()) == 1
