"""CPU tests of the dispersion search's cases (tests/dispersion_cases.py) from the model alone (tests/dispersion_model.py): every
recovery case recovers its planted pair; every case's margin, best metric over second best, is at least 1 + 64 x its largest
relative tolerance, so that holding the library's winner to the truth's is fair; both compositions agree with the definition as a
double loop; the float composition's own ratio to the bound is printed (and is small); the cases cover what the GPU tests need."""
import numpy as np
import pytest

import dispersion_cases as dc
import dispersion_model as dm

IDS = [c["what"] for c in dc.CASES]


@pytest.mark.parametrize("case", [c for c in dc.CASES if c["recovery"]], ids=[c["what"] for c in dc.CASES if c["recovery"]])
def test_recovery_cases_recover_their_planted_pair(case):
    t, f = dc.case_models(case)
    assert t["index"] == dc.planted_index(case) == f["index"]


@pytest.mark.parametrize("case", dc.CASES, ids=IDS)
def test_margin_stands_clear_of_the_tolerance(case):
    t, _ = dc.case_models(case)
    m, rel = dm.margin(t), dm.largest_relative_tolerance(t, case["n"])
    print("%s: margin %.5f, largest relative tolerance %.3g, winner %d" % (case["what"], m, rel, t["index"]))
    assert t["index"] >= 0 and rel < 1e-3
    assert m >= 1.0 + 64.0 * rel


@pytest.mark.parametrize("case", dc.CASES, ids=IDS)
def test_float_composition_lies_far_inside_the_bound(case):
    t, f = dc.case_models(case)
    o2, o4 = dm.ratios(f["row_sums"], f["sums"], t, case["n"])
    print("%s: f32 composition |f32 - truth| / tol: S2 %.4g, S4 %.4g" % (case["what"], o2, o4))
    assert o2 <= 0.05 and o4 <= 0.05
    assert f["index"] == t["index"]


@pytest.mark.parametrize("case", [c for c in dc.CASES if c["brute"]], ids=[c["what"] for c in dc.CASES if c["brute"]])
def test_both_compositions_agree_with_the_double_loop(case):
    X = dc.case_field(case)
    t, f = dc.case_models(case)
    rows, sums = dm.brute(X, case["a2"], case["a3"], case["depth"])
    np.testing.assert_allclose(t["row_sums"], rows, rtol=1e-10, atol=0)
    np.testing.assert_allclose(t["sums"], sums, rtol=1e-10, atol=0)
    tb = dict(t, row_sums=rows, sums=sums)   # the float composition against the double loop, by the stage's own tolerance
    o2, o4 = dm.ratios(f["row_sums"], f["sums"], tb, case["n"])
    assert o2 <= 0.05 and o4 <= 0.05


def test_the_cases_cover_what_the_gpu_tests_need():
    from fdoct_amd import dispersion
    assert sum(c["recovery"] for c in dc.CASES) == 4
    assert any(c["n"] == 4096 for c in dc.CASES)
    assert any(c["a2"][2] == 1 and c["a3"][2] == 1 for c in dc.CASES) and any(c["a2"][2] > 1 and c["a3"][2] == 1 for c in dc.CASES)
    assert any(c["depth"] == (0, c["n"]) for c in dc.CASES) and any(c["depth"][1] == 1 for c in dc.CASES) and any(c["depth"] == (0, 0) for c in dc.CASES)
    assert any(c["zero_row"] is not None for c in dc.CASES)
    assert {c["n"] % 3 == 0 for c in dc.CASES} == {True, False} and any(c["n"] % 5 == 0 for c in dc.CASES)
    for c in dc.CASES:   # the chunk seam: the full grid spans 15 chunks, the last one short
        p = dispersion.plan(c["a2"], c["a3"], c["rows"], c["n"], c["depth"])
        assert p["candidates"] == c["a2"][2] * c["a3"][2]
        if p["candidates"] == 117:
            assert (p["per_workgroup"], p["chunks"]) == (8, 15) and 117 % 8 == 5


def test_zero_row_sums_are_exact_zeros_with_zero_tolerance():
    case = next(c for c in dc.CASES if c["zero_row"] is not None)
    t, f = dc.case_models(case)
    tol_rows, _ = dm.tolerances(t, case["n"])
    r = case["zero_row"]
    assert np.all(t["row_sums"][r] == 0) and np.all(f["row_sums"][r] == 0) and np.all(tol_rows[r] == 0)
    assert np.all(tol_rows[[q for q in range(case["rows"]) if q != r]] > 0)
