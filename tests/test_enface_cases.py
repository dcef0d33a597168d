"""The catalogue of tests/enface_cases.py held to the condition each case's name promises, on the model alone (no GPU): a case
that stops exercising what it is there for fails here, not silently on the card."""
import numpy as np
import pytest

import enface_cases
import enface_model


def _m(name):
    c = enface_cases.case(name)
    return c, enface_model.model(c["V"], c["p"], c["S"])


def test_the_catalogue_names_the_required_cases_and_shapes():
    assert {"ties", "no crossing", "clipped", "negative", "last candidate", "relative"} <= set(enface_cases.NAMES)
    shapes = [enface_cases.case(n)["V"].shape for n in enface_cases.NAMES]
    assert {1, 3, 67, 130, 257} <= {s[2] for s in shapes}
    assert {1, 3, 70} <= {s[1] for s in shapes}
    assert {1, 2, 3} <= {s[0] for s in shapes}
    for n in enface_cases.NAMES:
        c = enface_cases.case(n)
        assert c["V"].dtype == np.float32 and np.all(np.isfinite(c["V"])), n
        assert c["S"] is None or (c["S"].shape == c["V"].shape and c["S"].dtype == np.float32), n
        again = enface_cases.case(n)
        assert np.array_equal(c["V"], again["V"]), n           # the catalogue is a function of the name


def test_ties_has_a_slab_maximum_that_occurs_twice():
    c, m = _m("ties")
    V, twice = c["V"], 0
    for s, (first, count) in enumerate(c["p"]["slabs"]):
        for r in range(V.shape[1]):
            slab = V[0, r, first:first + count]
            twice += int(np.sum(slab == m["max"][s, 0, r]) >= 2)
            assert m["argmax"][s, 0, r] == first + int(np.argmax(slab))
    assert twice >= 1


def test_no_crossing_has_rows_with_and_without_a_valid_neighbour():
    c, m = _m("no crossing")
    none = m["z0"] < 0
    assert none.any()
    assert (none & (m["surface"] >= 0)).any(), "no A-scan takes its neighbours' surface"
    assert (none & (m["surface"] < 0)).any(), "no A-scan is left without a surface"
    gone = m["surface"] < 0
    assert np.all(m["mean"][:, gone] == 0) and np.all(m["max"][:, gone] == 0) and np.all(m["argmax"][:, gone] == -1)


def test_clipped_has_slabs_cut_at_both_ends_and_emptied():
    c, m = _m("clipped")
    D = c["V"].shape[2]
    z = m["surface"].astype(np.int64)
    assert np.all(z >= 0)
    low = high = empty = False
    for s, (first, count) in enumerate(c["p"]["slabs"]):
        lo, hi = z + first, z + first + count
        low |= bool(np.any((lo < 0) & (hi > 0) & (m["n"][s] == np.minimum(hi, D))))
        high |= bool(np.any((hi > D) & (lo < D) & (lo >= 0) & (m["n"][s] == D - lo)))
        empty |= bool(np.any(((hi <= 0) | (lo >= D)) & (m["n"][s] == 0)))
    assert low and high and empty


def test_negative_is_below_zero_everywhere():
    c, m = _m("negative")
    assert np.all(c["V"] < 0)
    some = m["n"] > 0
    assert some.any() and np.all(m["max"][some] < 0) and np.all(m["mean"][some] < 0)
    assert (m["z0"] >= 0).any()


def test_last_candidate_lies_at_the_end_of_the_search_range():
    c, m = _m("last candidate")
    s0, cnt = c["p"]["search"]
    last = s0 + cnt - c["p"]["smooth"]
    assert m["z0"][0, 0] == last and m["z0"][0, 2] == last and 0 <= m["z0"][0, 1] < last


def test_relative_is_crossed_by_some_and_not_all_candidates():
    c, m = _m("relative")
    q = enface_model.resolve(c["p"], c["V"].shape[2])
    B = enface_model.box_sums(c["V"], q["s0"], q["s1"], q["smooth"])
    hits = (B >= np.float32(q["threshold"]) * B.max(axis=-1, keepdims=True)).sum(axis=-1)
    assert np.all(hits >= 1) and np.all(hits < B.shape[-1])
    assert len(np.unique(m["z0"])) > 10


def test_structure_differs_from_the_volume_and_far_slabs_skip_a_block():
    c, m = _m("structure")
    assert not np.array_equal(m["surface"], enface_model.model(c["V"], c["p"])["surface"])
    c, m = _m("far slabs")
    z = int(m["surface"][0, 0])
    lo = [z + f for f, _ in c["p"]["slabs"]]
    assert max(lo) // 256 - min(max(l, 0) for l in lo) // 256 >= 2      # a whole block of 256 depths between two slabs


@pytest.mark.parametrize("name", enface_cases.NAMES)
def test_no_case_holds_a_nan_or_exempts_a_pixel(name):
    c, m = _m(name)
    for k in ("mean", "max", "truth", "bound"):
        assert np.all(np.isfinite(m[k])), k
    assert m["mean"].shape == m["max"].shape == m["argmax"].shape == (len(c["p"]["slabs"]),) + c["V"].shape[:2]
