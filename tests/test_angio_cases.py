"""CPU tests of the angiography stage's specification and catalogue (tests/angio_model.py, tests/angio_cases.py): the float
composition and the truth against the definitions as plain loops, the exemption caps from the truth alone, what the three kinds of
speckle must give, the bulk correction, and the plan's geometry."""
import numpy as np
import pytest

import angio_cases as ac
import angio_model as am
from fdoct_amd import angiography

IDS = [c["what"] for c in ac.CASES]


@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=IDS)
def test_model_and_truth_against_the_definitions(i):
    c = ac.CASES[i]
    X, (f32, tr, tol, (ill, edge)) = ac.case_refs(i)
    kw = ac.case_args(c)
    b = am.brute(X, kw["repeats"], kw["win"], kw["bulk"])
    plain = am.model(X, truth=True, **dict(kw, min_power=0.0))
    for k in am.NAMES:
        # the truth and the loops are both double: they differ by the order of a few hundred terms
        scale = np.maximum(np.abs(b[k]), 1.0 if k in ("decorr", "cdecorr") else 0.0)
        assert np.all(np.abs(plain[k] - b[k]) <= 1e-11 * scale + 1e-300), k
    figs = am.check(f32, X, c["what"] + " (the float composition as the result)", refs=(f32, tr, tol, (ill, edge)), **kw)
    # the float composition itself within the tolerance derived for it
    for k, (g, o) in figs.items():
        assert g == o and g <= 1.0, (k, g)


@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=IDS)
def test_exemption_caps_hold_from_the_truth_alone(i):
    _, (_, _, _, (ill, edge)) = ac.case_refs(i)
    assert ill.sum() <= 0.01 * ill.size and edge.sum() <= 0.01 * edge.size, (int(ill.sum()), int(edge.sum()), ill.size)


def test_the_masked_cases_mask_some_pixels_and_not_all():
    for i, c in enumerate(ac.CASES):
        if c["min_power"] > 0:
            _, (_, tr, _, _) = ac.case_refs(i)
            below = tr["power"] < c["min_power"]
            assert 0.05 < below.mean() < 0.95, (c["what"], below.mean())


def test_independent_speckle_decorrelates_to_one_minus_pi_over_four():
    """Fully developed speckle: |X| is Rayleigh, E A = sqrt(pi) sigma / 2 and E I = sigma^2, so for independent frames E A_n A_{n+1} /
    E I = pi / 4 and decorr -> 1 - pi / 4.  The sampling error of Q over M = cnt (N - 1) terms: per term A_n A_{n+1} / sigma^2 has
    variance 1 - (pi / 4)^2 = 0.383 (standard deviation 0.62) and (I_n + I_{n+1}) / (2 sigma^2) has 0.5 (0.71); to first order the
    ratio's standard deviation is at most (0.62 + (pi / 4) 0.71) / sqrt(M) = 1.18 / sqrt(M).  Five of those bound every pixel whose
    window is whole (cnt = 256, N - 1 = 7: 0.139); the mean over those pixels lies within one."""
    i = ac.index("independent, N 8, 20 x 70, window 16 x 16")
    c = ac.CASES[i]
    _, (f32, tr, _, _) = ac.case_refs(i)
    whole = tr["cnt"] == 256
    assert whole.sum() >= 5 * 55
    sd = 1.18 / np.sqrt(256 * (c["repeats"] - 1))
    for out in (f32, tr):
        d = out["decorr"][0][whole]
        assert np.abs(d - (1 - np.pi / 4)).max() <= 5 * sd and abs(d.mean() - (1 - np.pi / 4)) <= sd, (d.min(), d.max(), d.mean())
    # ... and the complex contrast is close to 1: |sum of M random phasors| / M ~ 1 / sqrt(M)
    assert tr["cdecorr"][0][whole].min() > 1 - 6 / np.sqrt(256 * 7)


def test_static_speckle_gives_no_contrast():
    """The frames differ by the noise floor alone, NOISE / SIGMA = 0.004 in amplitude: decorr and cdecorr are of the order of its
    square against the mean intensity in the window, var / power^2 of twice its square."""
    i = ac.index("static, N 4, 2 groups of 17 x 65, window 3 x 5")
    _, (f32, tr, tol, _) = ac.case_refs(i)
    for out in (f32, tr):
        assert np.abs(out["decorr"]).max() < 2e-3 and np.abs(out["cdecorr"]).max() < 2e-3
        assert (out["var"] / out["power"] ** 2).max() < 2e-3
    for k in ("decorr", "cdecorr", "var"):
        assert np.all(np.abs(f32[k] - tr[k]) <= tol[k]), k
    v = ac.index("vessel, N 3, 2 groups of 17 x 65, window 3 x 5, min_power")
    _, (_, tv, _, _) = ac.case_refs(v)
    live = tv["power"] >= ac.CASES[v]["min_power"]
    left, right = np.zeros(live.shape, bool), np.zeros(live.shape, bool)
    left[..., :28], right[..., 37:] = True, True          # clear of the window's reach across the middle
    # (30 terms a pixel: the standard deviation of test_independent_speckle's bound is 0.215, as large as 1 - pi / 4 itself -- the mean tells)
    assert tv["decorr"][left & live].max() < 0.01 < 0.02 < tv["decorr"][right & live].min()
    assert abs(tv["decorr"][right & live].mean() - (1 - np.pi / 4)) < 0.03
    assert tv["cdecorr"][left & live].max() < 0.01 < 0.2 < tv["cdecorr"][right & live].min()


def test_the_bulk_correction_removes_the_bulk_phase():
    a, b, n = (ac.index("static, %s, N 4, 9 x 130, %s" % s) for s in (("bulk phase of +-pi", "corrected"), ("no bulk phase", "corrected"),
                                                                     ("bulk phase of +-pi", "not corrected")))
    (_, (fa, ta, tola, _)), (_, (fb, tb, tolb, _)), (_, (fn, tn, _, _)) = ac.case_refs(a), ac.case_refs(b), ac.case_refs(n)
    # the two fields are the same up to the rounding of X to float pairs, which the 4 u of every product covers
    assert np.all(np.abs(fa["cdecorr"] - tb["cdecorr"]) <= tola["cdecorr"] + tolb["cdecorr"])
    assert np.all(np.abs(ta["cdecorr"] - tb["cdecorr"]) <= tola["cdecorr"] + tolb["cdecorr"])
    assert np.abs(ta["cdecorr"]).max() < 2e-3 and np.median(tn["cdecorr"]) > 0.3 and np.median(fn["cdecorr"]) > 0.3
    # the other three outputs do not read the phase at all
    for k in ("var", "decorr", "power"):
        assert np.all(np.abs(fa[k] - fn[k]) <= 2 * tola[k]), k
    # the first order of tol_B / |B| holds: |B| >= 16 tol_B on the corrected cases
    first, cnt = ac.BULK_RANGE
    X, _ = ac.case_refs(a)
    Xg = np.asarray(X, np.complex128).reshape(1, 4, 9, 130)
    mag = (np.abs(Xg[:, :-1]) * np.abs(Xg[:, 1:]))[..., first:first + cnt].sum(-1)
    assert np.all(np.abs(ta["B"]) >= 16 * (cnt + 4) * am.U * mag)


PLAN = [((4, (3, 5), None), 8, 17, 65, (2, 8, 8, 0)), ((2, (1, 1), True), 64, 1000, 1024, (32, 32 * 63 * 16, 1024, 32 * 1000 * 8)),
        ((4, (16, 16), (3, 0)), 64, 1000, 1024, (16, 16 * 63 * 16, 1024, 16 * 3 * 1000 * 8)), ((2, (1, 1), None), 2, 1, 1, (1, 1, 1, 0)),
        ((64, (1, 1), None), 65536, 2, 3, (1024, 1024, 1024, 0)), ((2, (1, 1), None), 65536, 1, 1, (32768, 32768, 1024, 0))]


@pytest.mark.parametrize("case", PLAN, ids=[str(c[:4]) for c in PLAN])
def test_the_plans_geometry(case):
    (repeats, win, bulk), nframes, H, D, want = case
    p = angiography.plan(dict(repeats=repeats, win=win, bulk=bulk), nframes, H, D)
    assert (p["groups"], p["tiles"], p["workgroups"], p["workspace_bytes"]) == want
    assert am.geometry(nframes, repeats, H, D) == want[:3]


def test_the_placement_case_is_beyond_one_pass_for_every_card():
    for cus in (64, 104, 128, 228, 256, 304):
        n = ac.placement_groups(cus)
        assert ac.beyond(n, ac.resident(cus)) and 2 * n <= 65536
