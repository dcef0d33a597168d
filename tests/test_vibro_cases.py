"""CPU tests of the vibrometry stage's specification and catalogue (tests/vibro_model.py, tests/vibro_cases.py): the float
composition and the truth against the definition as plain loops, the exemption caps, the reference sums' conditioning, PHASE_STEP's
record, the double arithmetic's term against the float one, the chunk identities, and the plan's arithmetic against the library's."""
import numpy as np
import pytest

import vibro_cases as vc
import vibro_model as vm
from fdoct_amd import vibrometry

IDS = [c["what"] for c in vc.CASES]
SMALL = [i for i, c in enumerate(vc.CASES) if c["T"] * c["H"] * c["D"] <= 40000]


@pytest.mark.parametrize("i", SMALL, ids=[IDS[i] for i in SMALL])
def test_model_and_truth_against_the_definition(i):
    c = vc.CASES[i]
    X, (f32, tr, tol, (ill, edge)) = vc.case_refs(i)
    kw = dict(vc.case_args(c), min_power=0.0)
    kw.pop("chunk_steps")
    kw.pop("min_power")
    sub = X[:, :min(c["H"], 3)]
    b = vm.brute(sub, **kw)
    t = vm.model(sub, truth=True, **kw)
    for k in ("amp", "rms", "drift", "power"):
        scale = max(1.0, float(np.abs(b[k]).max())) if b[k].size else 1.0
        err = float(np.abs(t[k] - b[k]).max()) if b[k].size else 0.0
        print("%s: truth against brute, %s: %.3g (scale %.3g)" % (c["what"], k, err, scale))
        assert err <= 1e-9 * scale, (c["what"], k)
    # the composition holds its own tolerance on the pixels that are held
    keep = ~ill
    for k in ("amp", "rms", "drift", "power"):
        want = tol["truth"][k] if k != "power" else tr[k]
        if c["min_power"] > 0 and k != "power":
            keep_k = keep & ~edge
            want = np.where(tr["power"] < c["min_power"], 0, want)
        else:
            keep_k = keep if k != "power" else np.ones(keep.shape, bool)
        r = vm._ratio(f32[k], want, tol[k], keep_k)
        print("%s: the float composition's |model - truth| / tol, %s: %.4f" % (c["what"], k, r))
        assert r <= 1.0, (c["what"], k, r)


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=IDS)
def test_case_conditions(i):
    c = vc.CASES[i]
    X, (f32, tr, tol, (ill, edge)) = vc.case_refs(i)
    n = ill.size
    cap = max(1, n // 100) if n >= 100 else 0
    print("%s: %d of %d pixels exempt, %d at the mask's edge (cap %d)" % (c["what"], int(ill.sum()), n, int(edge.sum()), cap))
    assert int(ill.sum()) <= cap and int(edge.sum()) <= cap
    if c["ref"] is not None:
        C, tol_C = tol["C"], tol["tol_C"]
        zero = tol_C == 0
        assert (np.abs(C)[~zero] >= 16 * tol_C[~zero]).all() and (C[zero] == 0).all(), c["what"]
        if c["fld"].get("zero_row"):
            assert zero.sum() == 1
    # PHASE_STEP's record: the host's float arctan2 against double on the composition's own lag products
    d, re, im = vm.steps(X, c["ref"])
    worst = float(np.abs(d - np.arctan2(im.astype(np.float64), re.astype(np.float64))).max())
    print("%s: host arctan2, float against double: %.3g rad" % (c["what"], worst))
    assert worst <= vm.ATAN2F_HOST
    # the double arithmetic's term stays below 1/16 of the float term
    for k in ("rms", "amp"):
        if k == "amp" and not c["freq"]:
            continue
        ratio = float((tol["d_" + k] / tol["f_" + k]).max())
        print("%s: double term / float term, %s: %.3g" % (c["what"], k, ratio))
        assert ratio < 1.0 / 16
    if c["min_power"] > 0:
        below = tr["power"] < c["min_power"]
        assert below.sum() >= n // 10 and (~below).sum() >= n // 10, "both sides of the mask are to be populated"


def test_what_the_cases_are_there_for():
    by = {c["what"]: c for c in vc.CASES}
    ch = lambda c: vc.chunks(c["T"], c["H"], c["D"], c["chunk_steps"])   # noqa: E731
    assert [ch(by["T 8, 3 x 65, chunk %s" % s]) for s in ("1", "2", "3, line, Hann", "7 (one chunk)")] == [7, 4, 3, 1]
    assert ch(by["T 151, 2 x 130, chunk 50 (3 whole chunks)"]) == 3 and vm.chunks_of(151, 50)[-1] == (100, 150)
    assert ch(by["T 152, 2 x 130, chunk 50 (a fourth of one step)"]) == 4 and vm.chunks_of(152, 50)[-1] == (150, 151)
    assert ch(by["T 150, 2 x 130, chunk 50 (the third one short)"]) == 3 and vm.chunks_of(150, 50)[-1] == (100, 149)
    assert ch(by["T 200, 2 x 130, the rule (4 chunks), reference"]) == 4 and ch(by["T 20, 2 x 130, the rule (1 chunk)"]) == 1
    big = by["T 9, 50001 x 2, chunk 1, reference (two passes of both grids)"]
    assert vc.beyond(vc.series_items(big["T"], big["H"], big["D"], 1), vc.GRID_CAP) and vc.beyond(vc.ref_items(big["T"], big["H"]), vc.GRID_CAP)
    ramp = by["T 17, 3 x 67, a ramp of 2.5 rad a frame"]
    X, (_, tr, _, _) = vc.case_refs(vc.CASES.index(ramp))
    assert (np.abs(tr["drift"]) > 12 * np.pi).all() and np.abs(tr["d"]).max() < np.pi and np.abs(tr["d"]).min() > 1.5
    # the reference removes a common mode that the call without it does not
    i, j = (vc.CASES.index(by["T 40, 4 x 130, common mode of +-3 rad, %s" % s]) for s in ("reference", "no reference"))
    (Xi, ri), (Xj, rj) = vc.case_refs(i), vc.case_refs(j)
    assert np.array_equal(Xi, Xj)
    live = np.ones(130, bool)
    live[60:68] = False
    assert np.median(ri[1]["rms"][:, live]) < 1.0 < np.median(rj[1]["rms"][:, live])
    a = vc.field(40, 4, 130, 20, surface=(60, 8))[:, :, live]   # the same field without the common mode: what the reference restores
    quiet = vm.model(a, truth=True, freq=(vc.NU0,))
    assert np.abs(np.abs(ri[1]["amp"][0][:, live]) - np.abs(quiet["amp"][0])).max() < 0.05


@pytest.mark.parametrize("T,pixels,want", [(2, 1, (1, 1)), (64, 1000 * 1024, (63, 1)), (4096, 1024, (64, 64)), (65536, 1024, (1024, 64)),
                                           (200, 260, (64, 4)), (20, 260, (19, 1)), (66, 64, (64, 2)), (65, 64, (64, 1)), (65536, 1 << 24, (65535, 1)),
                                           (4096, 64 * 1024, (4095, 1)), (4096, 64 * 512, (2048, 2))])
def test_chunk_rule(T, pixels, want):
    cs = vm.chunk_rule(T, pixels)
    assert (cs, len(vm.chunks_of(T, cs))) == want
    p = vibrometry.plan(vibrometry.params(), T, 1, pixels)
    assert (p["chunk_steps"], p["chunks"]) == want


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=IDS)
def test_plan_agrees_with_the_restated_arithmetic(i):
    c = vc.CASES[i]
    p = vibrometry.plan(vibrometry.params(**vc.case_params(c)), c["T"], c["H"], c["D"])
    n = vc.chunks(c["T"], c["H"], c["D"], c["chunk_steps"])
    assert p["chunks"] == n and p["workgroups"] == vc.series_items(c["T"], c["H"], c["D"], c["chunk_steps"])
    nf, pixels = len(c["freq"]), c["H"] * c["D"]
    want = (c["T"] * c["H"] * 8 if c["ref"] is not None else 0) + (n * (5 + 2 * nf) * pixels * 8 if n > 1 else 0)
    want += (nf * c["T"] + n * (nf + 1) * 2 + 3 * (nf + 1)) * 16 if nf else 0
    assert p["workspace_bytes"] == want


def test_chunk_identities_do_not_depend_on_the_chunking():
    """Any chunking gives the one-chunk sums up to double rounding: the identities themselves, apart from the kernels."""
    X = vc.field(41, 2, 9, 99, drift=0.2)
    kw = dict(freq=(vc.NU0, 0.5), detrend=1, window=vm.HANN, scale=-3.0)
    one = vm.model(X, chunk_steps=40, **kw)
    for cs in (1, 2, 7, 13, 39):
        got = vm.model(X, chunk_steps=cs, **kw)
        for k in ("amp", "rms", "drift", "power"):
            assert np.abs(got[k].astype(np.complex128) - one[k]).max() <= 4e-6 * max(1.0, np.abs(one[k]).max()), (cs, k)
