"""CPU checks of tests/doppler_cases.py from tests/doppler_model.py alone: every case of the GPU tests keeps its exemptions under
1 % of its bins, keeps |B_truth| >= 16 tol_B on every row that is not exactly 0 where the bulk correction is on, has masked and
unmasked bins where min_power is set, and is passed by the float composition itself; the recorded arctan2 figure covers every
case; the tall batch's sizes hold their conditions for several CU counts."""
import numpy as np
import pytest

import doppler_cases as dc
import doppler_model as dm


@pytest.mark.parametrize("case", dc.CASES, ids=[c["what"] for c in dc.CASES])
def test_every_case_keeps_its_conditions(case):
    X, kw = dc.case_field(case), dc.case_args(case)
    geo = dict(axis=kw["axis"], lag=kw["lag"], win=kw["win"], bulk=kw["bulk"])
    ill, edge = dm.exemptions(X, min_power=kw["min_power"], **geo)
    print("%s: %d of %d bins exempt from the phase check, %d from the mask check" % (case["what"], ill.sum(), ill.size, edge.sum()))
    assert ill.sum() <= 0.01 * ill.size and edge.sum() <= 0.01 * edge.size
    tol = dm.tolerances(X, **geo)
    fl, tr = dm.model(X, **kw), dm.model(X, truth=True, **kw)
    if kw["bulk"]:
        live = tol["tol_B"] > 0
        assert np.all(np.abs(tol["B"][live]) >= 16 * tol["tol_B"][live])
        assert dm._ratio(fl["B"], tol["B"], tol["tol_B"]) <= 1.0
        if case["zero_row"]:
            assert (~live).any() and np.all(tol["B"][~live] == 0)
    if kw["min_power"] > 0:
        below = tr["power"] < kw["min_power"]
        assert 0.1 * below.size <= below.sum() <= 0.9 * below.size
    rR, rP = dm._ratio(fl["corr"], tr["corr"], tol["tol_R"]), dm._ratio(fl["power"], tr["power"], tol["tol_P"])
    print("%s: the float composition's own ratios: corr %.4f, power %.4f" % (case["what"], rR, rP))
    assert rR <= 1.0 and rP <= 1.0
    # the host's arctan2 in float against double, on the float composition's R
    R = fl["corr"]
    a32 = np.arctan2(R.imag, R.real)
    assert a32.dtype == np.float32
    worst = float(np.abs(dm.wrap(a32.astype(np.float64) - np.arctan2(R.imag.astype(np.float64), R.real.astype(np.float64)))).max())
    print("%s: |float32 arctan2 - float64 arctan2| <= %.3g rad" % (case["what"], worst))
    assert worst <= dm.ATAN2F_HOST


def test_case_list_covers_what_the_gpu_tests_are_asked_for():
    wins = {c["win"] for c in dc.CASES}
    assert {(1, 1), (1, 5), (3, 1), (3, 5), (4, 8), (32, 32)} <= wins
    assert {1, 67, 320} <= {c["D"] for c in dc.CASES} and any(c["D"] % dc.TILE_DEPTHS and c["D"] > dc.TILE_DEPTHS for c in dc.CASES)
    assert any(c["win"] == (32, 32) and (c["H"], c["D"]) == (40, 320) for c in dc.CASES)
    assert any(c["win"] == (32, 32) and (c["H"], c["D"]) == (12, 20) for c in dc.CASES)
    assert {1, 2} <= {c["lag"] for c in dc.CASES} and any(c["axis"] == dm.ASCANS and c["lag"] == c["H"] - 1 for c in dc.CASES)
    assert {dm.ASCANS, dm.FRAMES} == {c["axis"] for c in dc.CASES}
    assert any(c["bulk"] is True for c in dc.CASES) and any(isinstance(c["bulk"], tuple) for c in dc.CASES)
    assert any(c["bulk"] and c["zero_row"] for c in dc.CASES) and any(c["min_power"] > 0 for c in dc.CASES)
    for c in dc.CASES:
        assert 2 <= c["n"] <= 3 and 12 <= c["H"] <= 40 and float(np.float32(c["min_power"])) == c["min_power"]


@pytest.mark.parametrize("cus", [16, 64, 104, 228, 256, 304])
@pytest.mark.parametrize("axis", [dm.ASCANS, dm.FRAMES])
def test_tall_batch_sizes(axis, cus):
    n = dc.tall_frames(axis, cus)
    assert dc.tall_ok(axis, n, cus) and n % 3 == 0
    pi, pr = dc.tall_shape(axis, n)
    assert dc.tiles(pi, pr, dc.TALL_D) >= 1.5 * dc.grid_cap(cus) and pi * pr >= 1.5 * dc.grid_cap(cus)
    assert dc.base_ok(axis, cus)
    assert n * dc.TALL_H * dc.TALL_D * 8 < 64 << 20   # the tall batch stays small
