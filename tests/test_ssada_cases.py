"""CPU tests of the split-spectrum stage's specification and catalogue: tests/ssada_model.py agrees with the O(N^2) definition, the
float composition lies well inside the tolerance, every case's field has the zero rows it says and no other, the table
fdoct_ssada_band_table writes is the model's bit for bit, fdoct_ssada_plan's figures are the launch arithmetic restated in
tests/ssada_cases.py, and the ordering the GPU sanity test of the physics asserts holds in the model with the margin stated
there."""
import numpy as np
import pytest

import ssada_cases as sc
import ssada_model as sm
from fdoct_amd import ssada

IDS = [c["what"] for c in sc.CASES]


@pytest.mark.parametrize("i", sc.BRUTE, ids=[IDS[i] for i in sc.BRUTE])
def test_the_model_agrees_with_the_definition(i):
    c = sc.CASES[i]
    X, f, t = sc.case_refs(i)
    kw = sc.case_args(c)
    _, _, _, d0, dc = sm.resolve(c["N"], c["bands"], c["sigma"], c["support"], c["depth"])
    B = sm.layout(sm.brute(X, c["bands"], c["sigma"], c["support"]), c["repeats"], d0, dc)
    scale = np.abs(B).max() if np.abs(B).max() > 0 else 1.0
    assert np.abs(t["bands"] - B).max() <= 1e-11 * max(scale, np.abs(X).max()), "the truth and the definition disagree"
    row, bins = sm.band_ratios(f["bands"], t, c["N"])
    print("%s: the float composition's |f32 - truth| / tol: row %.4g, bin %.4g" % (c["what"], row, bins))
    assert row <= 0.5 and bins <= 0.5
    assert kw["repeats"] == c["repeats"]


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_every_case_has_the_zero_rows_it_says_and_its_models_have_their_shapes(i):
    c = sc.CASES[i]
    X, f, t = sc.case_refs(i)
    T, H, N = c["groups"] * c["repeats"], c["H"], c["N"]
    assert X.shape == (T, H, N) and X.dtype == np.complex64
    zero = {(int(a), int(b)) for a, b in zip(*np.nonzero(~X.any(axis=-1)))}
    assert zero == sc.zero_rows(c)
    _, _, _, d0, dc = sm.resolve(N, c["bands"], c["sigma"], c["support"], c["depth"])
    for m in (f, t):
        assert m["bands"].shape == (c["groups"], c["bands"], c["repeats"], H, dc)
        assert m["band_decorr"].shape == (c["groups"], c["bands"], H, dc) and m["decorr"].shape == m["power"].shape == (c["groups"], H, dc)
        assert all(np.isfinite(m[k]).all() for k in ("bands", "band_decorr", "decorr", "power"))
    assert f["bands"].dtype == np.complex64 and f["decorr"].dtype == np.float32 and f["power"].dtype == np.float32
    row, bins = sm.band_ratios(f["bands"], t, N)
    assert row <= 0.5 and bins <= 0.5, (row, bins)
    # a zero row's band A-scans are zero in both models (tolerance 0)
    for (fr, r) in sc.zero_rows(c):
        g, n = divmod(fr, c["repeats"])
        assert not f["bands"][g, :, n, r].any() and not t["bands"][g, :, n, r].any() and not t["norm"][g, :, n, r].any()


def test_the_catalogue_holds_what_its_header_lists():
    Ns = {c["N"] for c in sc.CASES}
    assert Ns == {16, 60, 1000, 1024, 4096}
    assert {c["bands"] for c in sc.CASES} == {1, 3, 4, 16}
    assert {c["repeats"] for c in sc.CASES} == {2, 3, 4} and {c["groups"] for c in sc.CASES} == {1, 2, 3}
    assert min(c["H"] for c in sc.CASES) == 1 and max(c["H"] for c in sc.CASES) == 17
    assert {c["win"] for c in sc.CASES} == {(1, 1), (3, 5), (16, 16)}
    depths = [c["depth"] for c in sc.CASES]
    assert (0, 0) in depths and any(d[1] == 1 for d in depths) and any(d[0] % 64 and d[1] % 2 for d in depths)
    assert any(d == (0, c["N"]) for d, c in zip(depths, sc.CASES))
    supports = [(c["support"], c["bands"]) for c in sc.CASES]
    assert any(s == (0, 0) for s, _ in supports) and any(0 < s[1] < M for s, M in supports) and any(s[0] > 0 and s[1] >= M for s, M in supports)
    small = [c for c in sc.CASES if c["win"] == (16, 16)]
    assert any(c["H"] < 16 and sm.resolve(c["N"], c["bands"], c["sigma"], c["support"], c["depth"])[4] < 16 for c in small)
    assert any(c["fld"].get("zero_row") for c in sc.CASES) and any(c["fld"].get("zero_frame") for c in sc.CASES)


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_the_librarys_table_is_the_models_bit_for_bit(i):
    c = sc.CASES[i]
    p = ssada.params(n=c["N"], **sc.case_args(c))
    got = ssada.band_table(p, c["N"])
    want = sm.band_table(c["N"], c["bands"], c["sigma"], c["support"])
    assert got.dtype == np.float32 and got.shape == want.shape == (c["bands"], c["N"])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    k0, kc, sg, _, _ = sm.resolve(c["N"], c["bands"], c["sigma"], c["support"])
    assert p.sigma == sg
    assert not got[:, :k0].any() and not got[:, k0 + kc:].any() and (got[:, k0:k0 + kc] >= 0).all()


def test_the_identity_table_rounds_to_one():
    t = ssada.band_table(dict(repeats=2, bands=1, sigma=1e12), 1000)
    assert (t == np.float32(1)).all()
    assert (sm.band_table(1000, 1, 1e12) == np.float32(1)).all()


PLANS = [(c, 0) for c in sc.CASES] + [(sc.CASES[2], 3 * sc.group_share(3, 3, 17, 11) // 2), (sc.CASES[1], sc.group_share(2, 16, 5, 16))]


@pytest.mark.parametrize("c,cap", PLANS, ids=["%s, cap %d" % (c["what"], cap) for c, cap in PLANS])
def test_plan_is_the_launch_arithmetic(c, cap):
    T = c["groups"] * c["repeats"]
    kw = dict(sc.case_args(c), max_workspace_bytes=cap)
    got = ssada.plan(kw, T, c["H"], c["N"])
    want = sc.plan(T, c["repeats"], c["bands"], c["H"], c["N"], c["depth"], cap)
    assert got == want
    assert got["lds_bytes"] == 24 * c["N"] and got["groups_per_pass"] * got["passes"] >= got["groups"]


def test_the_capped_grid_case_is_beyond_one_pass_for_several_cards():
    for cus in (64, 104, 256, 304):
        for dc in (8, 3):
            H = sc.grid_ascans(cus, dc)
            assert sc.beyond(2 * H, sc.resident(cus)) and sc.beyond(H * dc, sc.resident(cus) * sc.BLOCK)
            assert H * dc <= 1 << 24


def test_the_physics_ordering_holds_in_the_model():
    X = sc.physics_field()
    sc.physics_check({M: sm.model(X, bands=M, **sc.PHYS)["decorr"] for M in (1, 4)}, "the float composition")
    sc.physics_check({M: sm.model(X, bands=M, truth=True, **sc.PHYS)["decorr"] for M in (1, 4)}, "the truth")
