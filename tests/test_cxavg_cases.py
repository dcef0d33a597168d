"""CPU tests of the coherent-averaging stage's specification (tests/cxavg_model.py) and catalogue (tests/cxavg_cases.py): the float
composition against the truth against the definitions as plain loops on every case; the conditioning rule that stands in for
exemptions; that the catalogue holds what tests/test_gpu_cxavg.py is meant to exercise; and what the stage is for -- on a static
field whose frames carry phases of their own the aligned average keeps the signal and the unaligned one loses it, and on
independent speckle the coherent average falls by sqrt(N) -- with every margin taken from the truth model on the same field."""
import numpy as np
import pytest

import cxavg_cases as cc
import cxavg_model as cm

IDS = [c["what"] for c in cc.CASES]


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=IDS)
def test_model_truth_and_brute_agree_and_the_case_is_well_conditioned(i):
    c = cc.CASES[i]
    X, (f32, tol) = cc.case_refs(i)
    kw = cc.case_args(c)
    tr = tol["truth"]
    br = cm.brute(X, **kw)
    for k in cm.NAMES:
        assert f32[k].shape == tr[k].shape == br[k].shape == ((X.shape[0] - c["repeats"]) // (c["stride"] or c["repeats"]) + 1, c["H"], c["D"])
        scale = max(float(np.abs(tr[k]).max()), 1e-300)
        assert float(np.abs(br[k] - tr[k]).max()) <= 1e-12 * scale, k              # two evaluations in double
        assert cm._ratio(f32[k], tr[k], tol[k]) <= 1.0, k                          # the float composition lies within its own tolerance
    # the conditioning rule: |C| is exactly 0 or at least 16 tol_C, for every (group, repeat, A-scan)
    assert tol["condition"] >= cm.CONDITION, tol["condition"]
    # check() passes on the model's own output and refuses one that is off by twice the tolerance in one pixel
    cm.check(f32, X, c["what"], refs=(f32, tol), **kw)
    bad = {k: v.copy() for k, v in f32.items()}
    at = np.unravel_index(int(np.argmax(tol["mag"])), tol["mag"].shape)
    bad["mag"][at] = np.float32(tr["mag"][at] + 2.0 * tol["mag"][at] + 1e-3 * tr["mag"][at])
    with pytest.raises(AssertionError):
        cm.check(bad, X, c["what"], refs=(f32, tol), **kw)


def test_zeros_give_exact_zeros_and_unit_phasors():
    for what, zero_ref in (("the ref a frame of zeros, N 4, 3 x 130, align 1", True), ("the ref a frame of zeros, N 4, 2 x 1100, align 2 (streaming)", True),
                           ("a repeat a frame of zeros, N 4, 3 x 130, align 1", False), ("a repeat a frame of zeros, N 4, 3 x 130, align 2", False)):
        i = cc.index(what)
        c = cc.CASES[i]
        X, (f32, tol) = cc.case_refs(i)
        C = tol["truth"]["C"]
        n = c["fld"]["zero_frame"][1]
        assert np.all(X[n] == 0)
        if zero_ref:
            assert n == c["ref"] and np.all(C == 0)                                # every phasor is 1: the plain complex mean
            plain = cm.model(X, **dict(cc.case_args(c), align=0))
            assert all(np.array_equal(f32[k], plain[k]) for k in cm.NAMES)
        else:
            assert n != c["ref"] and np.all(C[:, n] == 0) and np.all(np.delete(C, [n, c["ref"]], axis=1) != 0)
    i = cc.index("an A-scan of the ref zeros, N 3, 2 groups of 4 x 130, align 1")
    X, (f32, tol) = cc.case_refs(i)
    C = tol["truth"]["C"]
    assert np.all(C[1, :, 2] == 0) and np.count_nonzero(C == 0) == 3              # that A-scan's three sums and no other


def test_the_catalogue_covers_what_the_gpu_tests_are_for():
    cs = cc.CASES
    depths = {c["D"] for c in cs}
    assert {1, 255, 256, 257, 513} <= depths and any(c["H"] == 1 for c in cs)
    assert {2, 64} <= {c["repeats"] for c in cs}
    assert {0, 1, 2} == {c["align"] for c in cs}
    # each side of the forms' boundary, by the restated launch arithmetic: a register case whose depths + 1 is a streaming case,
    # every instantiation of the register form (2, 4, 8, 16 repeats held), one of them with fewer repeats than it holds, and every
    # align mode in both forms
    reg = [c for c in cs if cc.case_form(c) == cm.FORM_REGISTER]
    stream = [c for c in cs if cc.case_form(c) == cm.FORM_STREAMING]
    for N, D in ((8, 512), (2, 2048)):
        assert any((c["repeats"], c["D"]) == (N, D) for c in reg) and any((c["repeats"], c["D"]) == (N, D + 1) for c in stream)
        assert cm.register_slots(N, D) * (-(-D // cm.BLOCK)) == cm.REG_PAIRS
    assert {cm.register_slots(c["repeats"], c["D"]) for c in reg} == {2, 4, 8, 16}
    assert any(cm.register_slots(c["repeats"], c["D"]) > c["repeats"] for c in reg)
    assert {0, 1, 2} == {c["align"] for c in reg} == {c["align"] for c in stream}
    # more than one pair a thread and a tail, in both forms
    assert any(c["D"] > 2 * cm.BLOCK and c["D"] % cm.BLOCK for c in reg) and any(c["D"] > 2 * cm.BLOCK and c["D"] % cm.BLOCK for c in stream)
    # the ref first, last and in the middle
    assert any(c["ref"] == 0 for c in cs) and any(c["ref"] == c["repeats"] - 1 for c in cs) and any(0 < c["ref"] < c["repeats"] - 1 for c in cs)
    # a range that ends at the last depth, one of a single depth, and a half-range
    ranges = [cm.resolve_range(c["align"], c["align_range"], c["D"]) + (c["D"],) for c in cs if c["align"] and c["align_range"] != (0, 0)]
    assert any(f + n == D and f > 0 for f, n, D in ranges) and any(n == 1 for f, n, D in ranges) and any(f == 0 and n < D for f, n, D in ranges)
    # zeros as the ref, as another repeat, as one A-scan
    zf = [c for c in cs if "zero_frame" in c["fld"]]
    assert any(c["fld"]["zero_frame"][1] == c["ref"] for c in zf) and any(c["fld"]["zero_frame"][1] != c["ref"] for c in zf)
    assert any("zero_row" in c["fld"] for c in cs)
    # sliding: stride 1 with N 3 over six frames
    assert any(c["stride"] == 1 and c["repeats"] == 3 and c["frames"] == (1, 6) for c in cs)
    assert any(c["stride"] not in (None, c["repeats"]) and c["align"] == 2 for c in cs)
    # odd depths: rows that are only 8-byte aligned
    assert sum(c["D"] % 2 for c in cs) >= 5


def test_placement_arithmetic():
    for cus in (256, 304, 64, 1):
        n = cc.placement_items(cus)
        assert cc.ac.beyond(n, cc.resident(cus))
    assert cm.geometry(64, 4, None, 1000, 1024, 1) == (16, cm.FORM_REGISTER, 1024, 0)
    assert [cm.register_slots(n, d) for n, d in ((2, 2048), (2, 2049), (3, 1024), (5, 512), (5, 513), (16, 256), (16, 257), (17, 1), (64, 1))] == [2, 0, 4, 8, 0, 16, 0, 0, 0]
    assert cm.geometry(64, 4, 1, 1000, 1025, 2, cus=64) == (61, cm.FORM_STREAMING, 256, 61 * 4 * 1001 * 8)


# ---- what the stage is for -------------------------------------------------------------------------------------------------------
STATIC = dict(groups=2, N=4, H=5, D=257, seed=1)


def _static(align):
    X = cc.ac.field(STATIC["groups"], STATIC["N"], STATIC["H"], STATIC["D"], STATIC["seed"], bulk_phase=np.pi)
    kw = dict(repeats=STATIC["N"], align=align)
    return cm.model(X, **kw), cm.model(X, truth=True, **kw), cm.tolerances(X, **kw)


def test_alignment_keeps_a_static_signal_and_its_absence_loses_it():
    """The field is the same speckle in every repeat, amplitude sigma = 1000 a component, plus noise of 4 a component, and every
    (frame, A-scan) has a phase of its own in [-pi, pi].  Aligned, the N repeats add in phase: |Z| = |X| up to the noise, which the
    truth model gives.  Unaligned they add as N random unit phasors: E |sum|^2 = N, so mag / incoh is about 1 / sqrt(N) = 0.5, and
    no single pixel can exceed 1."""
    f32, tr, tol = _static(1)
    ratio_t = tr["mag"] / tr["incoh"]
    assert ratio_t.min() > 0.5 and np.median(ratio_t) > 0.99 and np.median(tr["coh"]) > 0.99        # the truth itself: the noise costs under 1 %
    margin = (tol["mag"] / tr["incoh"] + tr["mag"] * tol["incoh"] / tr["incoh"] ** 2).max()         # first order, from the truth's tolerances
    assert np.abs(f32["mag"] / f32["incoh"] - ratio_t).max() <= margin
    assert np.abs(f32["coh"] - tr["coh"]).max() <= tol["coh"].max() and np.median(f32["coh"]) > 0.99
    g32, gr, gtol = _static(0)
    assert np.array_equal(g32["incoh"], f32["incoh"])                                               # the same frames, the same moduli
    loss_t = np.median(gr["mag"] / gr["incoh"])
    assert 0.25 < loss_t < 0.75                                                                     # about 1 / sqrt(4)
    assert abs(np.median(g32["mag"] / g32["incoh"]) - loss_t) <= (gtol["mag"] / gr["incoh"]).max() + (gr["mag"] * gtol["incoh"] / gr["incoh"] ** 2).max()
    assert np.median(g32["coh"]) < 0.75 and np.median(f32["mag"]) > 1.3 * np.median(g32["mag"])


@pytest.mark.parametrize("N", [4, 16])
def test_independent_speckle_falls_by_the_square_root_of_the_repeats(N):
    """Independent circular Gaussian speckle, unaligned: Z is the mean of N independent circular Gaussians of variance s^2, itself
    one of variance s^2 / N, so E|Z| = E|X| / sqrt(N) exactly.  Over P pixels the mean of a Rayleigh variable (coefficient of
    variation 0.523) is known to 0.523 / sqrt(P); the two means are nearly independent, so five standard deviations of their ratio
    is 5 x 0.523 sqrt(1 / P + 1 / (N P)) -- the speckle statistics of the case, nothing of the code."""
    H, D = 8, 512
    X = cc.ac.field(1, N, H, D, 77, kind="independent")
    kw = dict(repeats=N, align=0)
    f32, tr, tol = cm.model(X, **kw), cm.model(X, truth=True, **kw), cm.tolerances(X, **kw)
    P = H * D
    allow = 5 * 0.523 * np.sqrt(1.0 / P + 1.0 / (N * P))
    fall_t = tr["mag"].mean() / tr["incoh"].mean() * np.sqrt(N)
    assert abs(fall_t - 1) <= allow, (fall_t, allow)
    fall = f32["mag"].astype(np.float64).mean() / f32["incoh"].astype(np.float64).mean() * np.sqrt(N)
    assert abs(fall - fall_t) <= (tol["mag"].mean() / tr["incoh"].mean() + tr["mag"].mean() * tol["incoh"].mean() / tr["incoh"].mean() ** 2) * np.sqrt(N)
    # aligned to a ref the fall is smaller -- the ref's own term is always in phase with itself -- but the floor still drops
    al = cm.model(X, truth=True, repeats=N, align=1)
    assert fall_t <= al["mag"].mean() / al["incoh"].mean() * np.sqrt(N) < np.sqrt(N) * 0.75
