"""The float32 model of the en-face stage (tests/enface_model.py) on the CPU: against an independent loop over scalars on every
catalogue case -- integer outputs and the maximum equal, the mean within the derived bound of the float64 truth -- and the order of
a slab's sum against a 70-depth row worked by hand."""
import numpy as np
import pytest

import enface_cases
import enface_model

F = np.float32


@pytest.mark.parametrize("name", enface_cases.NAMES)
def test_model_agrees_with_the_brute_force_loop(name):
    c = enface_cases.case(name)
    m, b = enface_model.model(c["V"], c["p"], c["S"]), enface_model.brute(c["V"], c["p"], c["S"])
    for k in ("z0", "surface"):
        assert (k in m) == (k in b)
        if k in m:
            assert np.array_equal(m[k], b[k]), k
    assert np.array_equal(m["argmax"], b["argmax"])
    assert np.array_equal(m["max"], b["max"])
    assert np.allclose(m["truth"], b["mean"], rtol=1e-12, atol=0)        # two float64 sums of the same terms
    assert np.all(np.abs(m["mean"].astype(np.float64) - m["truth"]) <= m["bound"])
    empty = m["n"] == 0
    assert np.all(m["mean"][empty] == 0) and np.all(m["max"][empty] == 0) and np.all(m["argmax"][empty] == -1)


def test_the_order_of_a_slab_sum_on_a_hand_worked_row():
    # 70 depths, the slab [1, 70): partial l holds depths 4 l .. 4 l + 3, so lanes 0 .. 16 hold four depths each (lane 0 three: depth 0
    # lies outside) and lane 17 depths 68 and 69.  Values that are no short binary fractions make the roundings depend on the order.
    v = np.array([F(0.1) * F(b % 7 + 1) + F(b) * F(1e-3) for b in range(70)], F)
    v[0] = F(12345.0)                                                   # outside the slab
    p = [F(0)] * 64
    for lane in range(18):
        for b in range(4 * lane, min(4 * lane + 4, 70)):
            if b >= 1:
                p[lane] = F(p[lane] + v[b])
    for k in (32, 16, 8, 4, 2, 1):
        for lane in range(k):
            p[lane] = F(p[lane] + p[lane + k])
    got = enface_model.slab_sums(v[None, :], np.array([1]), np.array([70]))
    assert got.dtype == F and got[0] == p[0]
    # the order matters here: the plain left-to-right sum gives other bits
    acc = F(0)
    for b in range(1, 70):
        acc = F(acc + v[b])
    assert acc != p[0]
    m = enface_model.model(v[None, None, :], dict(slabs=[(1, 69)]))
    assert m["mean"][0, 0, 0] == F(p[0] / F(69))


def test_the_order_spans_blocks_of_256_depths():
    # depths 4 and 260 share partial 1: it adds them in increasing depth before the butterfly sees it
    v = np.zeros(300, F)
    v[4], v[260], v[8] = F(2.0) ** 24, F(1.0), F(1.0)
    # partial 1: 2^24 + 1 -> 2^24 (rounded); partial 2: 1; the butterfly adds 2^24 + 1 -> 2^24.  Left to right would give the same here,
    # but 1 + 1 first would give 2^24 + 2
    assert enface_model.slab_sums(v[None, :], np.array([0]), np.array([300]))[0] == F(2.0) ** 24


def test_the_bound_is_the_headers():
    V = np.ones((1, 1, 100), F)
    m = enface_model.model(V, dict(slabs=[(10, 50)]))
    assert m["n"][0, 0, 0] == 50 and m["bound"][0, 0, 0] == 1.01 * 50 * 2.0 ** -24 and m["truth"][0, 0, 0] == 1.0
