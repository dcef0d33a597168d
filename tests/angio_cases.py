"""The fields and cases of the angiography stage's tests (tests/test_angio_cases.py on the CPU, tests/test_gpu_angio.py on the GPU),
and the launch arithmetic of the stage (fdoct_angio_kernels.h) restated next to them, as pure functions.

Fields are generated directly as complex64, no chain in front: per group a fully developed speckle field (circular complex
Gaussian, so |X| is Rayleigh) that is the same in every repeat (static), drawn anew in every repeat (independent), or static on
the first half of the depths and independent on the second (a "vessel"); additive noise of a few counts in every frame, the floor
that keeps a static pixel's variance and every denominator away from an exact 0; optionally a frame or one A-scan of one frame
that is exactly 0, and a bulk phase per (frame, A-scan) that every depth shares."""
import functools

import numpy as np

import angio_model as am

SIGMA, NOISE = 1000.0, 4.0


def field(groups, repeats, H, D, seed, kind="static", zero_frame=None, zero_row=None, bulk_phase=0.0):
    """X (groups * repeats, H, D) complex64.  kind: static | independent | vessel.  zero_frame: (group, repeat); zero_row: (group,
    repeat, A-scan); bulk_phase: the half-width of the random phase per (frame, A-scan), applied last."""
    rng = np.random.default_rng(seed)

    def speckle(*shape):
        return (rng.normal(0, SIGMA, shape) + 1j * rng.normal(0, SIGMA, shape)) / np.sqrt(2.0)

    fixed = np.broadcast_to(speckle(groups, 1, H, D), (groups, repeats, H, D))
    fresh = speckle(groups, repeats, H, D)
    moving = np.zeros((H, D), bool)
    if kind == "independent":
        moving[:] = True
    elif kind == "vessel":
        moving[:, D // 2:] = True
    else:
        assert kind == "static"
    X = np.where(moving, fresh, fixed) + (rng.normal(0, NOISE, fresh.shape) + 1j * rng.normal(0, NOISE, fresh.shape))
    phase = rng.uniform(-1.0, 1.0, (groups, repeats, H, 1))          # drawn always, so that a case with and one without share the speckle
    X = X * np.exp(1j * bulk_phase * phase)
    if zero_frame is not None:
        X[zero_frame[0], zero_frame[1]] = 0
    if zero_row is not None:
        X[zero_row[0], zero_row[1], zero_row[2]] = 0
    return X.reshape(groups * repeats, H, D).astype(np.complex64)


def _case(what, groups, repeats, H, D, seed, win=(1, 1), bulk=None, min_power=0.0, **fld):
    return dict(what=what, groups=groups, repeats=repeats, H=H, D=D, seed=seed, win=win, bulk=bulk, min_power=float(min_power), fld=fld)


BULK_RANGE = (10, 100)
CASES = [
    # the three kinds of speckle
    _case("static, N 4, 2 groups of 17 x 65, window 3 x 5", 2, 4, 17, 65, 1, win=(3, 5)),
    _case("independent, N 8, 20 x 70, window 16 x 16", 1, 8, 20, 70, 2, win=(16, 16), kind="independent"),
    _case("vessel, N 3, 2 groups of 17 x 65, window 3 x 5, min_power", 2, 3, 17, 65, 3, win=(3, 5), kind="vessel", min_power=0.7e6),
    _case("vessel, N 3, 17 x 65, window 5 x 5, bulk over all depths", 1, 3, 17, 65, 4, win=(5, 5), kind="vessel", bulk=True),
    # zeros
    _case("a frame of zeros, N 4, 18 x 66, window 1 x 1", 1, 4, 18, 66, 5, zero_frame=(0, 2)),
    _case("a frame of zeros, N 4, 18 x 66, window 3 x 5, bulk", 1, 4, 18, 66, 5, win=(3, 5), bulk=(3, 40), zero_frame=(0, 2)),
    _case("a row of zeros, N 3, 2 groups of 9 x 67, window 3 x 5, bulk", 2, 3, 9, 67, 6, win=(3, 5), bulk=(0, 0), kind="vessel", zero_row=(1, 1, 5)),
    # the bulk phase: with it and the correction, without it and with the correction, with it and without the correction
    _case("static, bulk phase of +-pi, N 4, 9 x 130, corrected", 1, 4, 9, 130, 7, win=(3, 5), bulk=BULK_RANGE, bulk_phase=np.pi),
    _case("static, no bulk phase, N 4, 9 x 130, corrected", 1, 4, 9, 130, 7, win=(3, 5), bulk=BULK_RANGE),
    _case("static, bulk phase of +-pi, N 4, 9 x 130, not corrected", 1, 4, 9, 130, 7, win=(3, 5), bulk_phase=np.pi),
    # repeats
    _case("independent, N 2, 3 groups of 5 x 67, window 1 x 1", 3, 2, 5, 67, 8, kind="independent"),
    _case("vessel, N 2, 17 x 65, window 3 x 5", 1, 2, 17, 65, 9, win=(3, 5), kind="vessel"),
    _case("vessel, N 8, 6 x 70, window 2 x 4 (even sizes)", 1, 8, 6, 70, 10, win=(2, 4), kind="vessel"),
    # tile seams and windows beyond the image
    _case("vessel, N 3, 16 x 64 exactly, window 3 x 5", 1, 3, 16, 64, 11, win=(3, 5), kind="vessel"),
    _case("vessel, N 3, 1 x 130, window 3 x 5, bulk", 1, 3, 1, 130, 12, win=(3, 5), kind="vessel", bulk=True),
    _case("independent, N 3, 33 x 1, window 5 x 3", 1, 3, 33, 1, 13, win=(5, 3), kind="independent"),
    _case("independent, N 3, 2 groups of 2 x 3, window 16 x 16", 2, 3, 2, 3, 14, win=(16, 16), kind="independent"),
    _case("vessel, N 4, 33 x 130, window 16 x 1, min_power", 1, 4, 33, 130, 15, win=(16, 1), kind="vessel", min_power=0.9e6),
    _case("vessel, N 4, 18 x 129, window 1 x 16", 1, 4, 18, 129, 16, win=(1, 16), kind="vessel"),
]


def index(what):
    return [c["what"] for c in CASES].index(what)


def case_field(c):
    return field(c["groups"], c["repeats"], c["H"], c["D"], c["seed"], **c["fld"])


def case_args(c):
    """The keywords of angio_model's functions, and of fdoct_amd.angiography.params."""
    return dict(repeats=c["repeats"], win=c["win"], bulk=c["bulk"], min_power=c["min_power"])


@functools.lru_cache(maxsize=None)
def case_refs(i):
    """(X, (model, truth, tolerances, exemptions)) of CASES[i]: computed once, shared, never written to."""
    c = CASES[i]
    X = case_field(c)
    kw = case_args(c)
    tol = am.tolerances(X, **kw)
    refs = (am.model(X, **kw), am.model(X, truth=True, **kw), tol, am.exemptions(X, tol=tol, **kw))
    X.setflags(write=False)
    return X, refs


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
def resident(cus):
    """resident_blocks(CUs, 16 waves per CU, 256): the cap of the stage's grid."""
    return cus * am.BLOCKS_PER_CU


def placement_groups(cus):
    """Groups of one tile each for one and a half passes of the capped grid and a partial one."""
    n = -(-3 * resident(cus) // 2) + 1
    while n % resident(cus) == 0:
        n += 1
    return n


def beyond(items, stride):
    """At least one and a half passes of `stride` items, the last one partial."""
    return 2 * items >= 3 * stride and items % stride != 0
