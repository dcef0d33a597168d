"""The fields and cases of the split-spectrum stage's tests (tests/test_ssada_cases.py on the CPU, tests/test_gpu_ssada.py on the
GPU), and the launch arithmetic of the stage (fdoct_ssada_kernels.h, fdoct_ssada.cpp: plan_ssada) restated next to them, as pure
functions.

Fields are angio_cases.field's with D = N: complex64 speckle of the full transform length, static, independent or a vessel, with
optionally a frame or one A-scan of one frame that is exactly 0.

The shapes are the smallest at which each thing can go wrong: N = 16 is one radix-16 pass, 60 = 3 4 5 and 1000 = 2^3 5^3 the mixed
radices, 1024 several butterflies a thread, 4096 the LDS grant and the longest plan; A-scans 1 .. 17, repeats 2 .. 4, groups 1 .. 3,
bands 1, 3, 4 and 16; depth ranges the default, an offset that is no multiple of 64 with an odd count, a count of 1 and the whole
of N; supports the whole spectrum, an inner range and a range of fewer bins than bands; windows 1 x 1, 3 x 5 and 16 x 16 on an
image smaller than the window."""
import functools

import numpy as np

import angio_cases as ac
import ssada_model as sm

DEFAULT_WORKSPACE = 2 << 30
PLAN_CUS = 256          # what fdoct_ssada_plan, which has no handle, takes for the card
BLOCK = 256
BLOCKS_PER_CU = 8       # kSsaWavesPerCu / 4: the cap of the split and mean kernels' grids


def _case(what, N, groups, repeats, H, bands, seed, sigma=None, support=(0, 0), depth=(0, 0), win=(1, 1), min_power=0.0, **fld):
    return dict(what=what, N=N, groups=groups, repeats=repeats, H=H, bands=bands, seed=seed, sigma=sigma, support=support, depth=depth, win=win,
                min_power=float(min_power), fld=fld)


CASES = [
    _case("N 16, 1 band, 1 A-scan, R 2, window 1 x 1", 16, 1, 2, 1, 1, 1),
    _case("N 16, 16 bands, 3 groups of 5, R 2, all of N, window 3 x 5", 16, 3, 2, 5, 16, 2, depth=(0, 16), win=(3, 5), kind="independent"),
    _case("N 60, 3 bands, 2 groups of 17, R 3, depths 7..17, window 3 x 5", 60, 2, 3, 17, 3, 3, depth=(7, 11), win=(3, 5), kind="vessel"),
    _case("N 60, 4 bands on a support of 3 bins, one depth, a row of zeros", 60, 2, 2, 4, 4, 4, support=(20, 3), depth=(29, 1), zero_row=(1, 0, 2)),
    _case("N 60, 4 bands, 2 x 5 image, window 16 x 16", 60, 1, 4, 2, 4, 5, depth=(3, 5), win=(16, 16), kind="independent"),
    _case("N 1000, 4 bands on bins 100..799, 3 A-scans, R 4, window 3 x 5", 1000, 1, 4, 3, 4, 6, support=(100, 700), win=(3, 5), kind="vessel"),
    _case("N 1000, 3 bands, sigma 40, R 2, depths 65..193, min_power", 1000, 2, 2, 2, 3, 7, sigma=40.0, depth=(65, 129), min_power=7.0e4, kind="vessel"),
    _case("N 1024, 4 bands, 2 groups of 4, R 2, depths 65..193, a frame of zeros", 1024, 2, 2, 4, 4, 8, depth=(65, 129), win=(3, 5), kind="vessel",
          zero_frame=(1, 1)),
    _case("N 4096, 3 bands, 2 A-scans, R 2, window 1 x 1", 4096, 1, 2, 2, 3, 9, kind="independent"),
    _case("N 4096, 1 band, all of N, 1 A-scan, R 3", 4096, 1, 3, 1, 1, 10, depth=(0, 4096), win=(3, 5)),
]
BRUTE = [0, 1, 2, 3, 4]   # the cases small enough for the O(N^2) definition


def index(what):
    return [c["what"] for c in CASES].index(what)


def case_field(c):
    return ac.field(c["groups"], c["repeats"], c["H"], c["N"], c["seed"], **c["fld"])


def case_args(c):
    """The keywords of ssada_model's functions, and (with n) of fdoct_amd.ssada.params."""
    return dict(repeats=c["repeats"], bands=c["bands"], sigma=c["sigma"], support=c["support"], depth=c["depth"], win=c["win"], min_power=c["min_power"])


def zero_rows(c):
    """The (frame, A-scan) rows the case says are zero."""
    f = c["fld"]
    rows = set()
    if f.get("zero_frame") is not None:
        g, n = f["zero_frame"]
        rows |= {(g * c["repeats"] + n, r) for r in range(c["H"])}
    if f.get("zero_row") is not None:
        g, n, r = f["zero_row"]
        rows.add((g * c["repeats"] + n, r))
    return rows


@functools.lru_cache(maxsize=None)
def case_refs(i):
    """(X, model, truth) of CASES[i]: computed once, shared, never written to."""
    c = CASES[i]
    X = case_field(c)
    kw = case_args(c)
    refs = (X, sm.model(X, **kw), sm.model(X, truth=True, **kw))
    X.setflags(write=False)
    return refs


# ---- the sanity case of the physics ------------------------------------------------------------------------------------------------
PHYS = dict(repeats=4, sigma=8.0, depth=(0, 256), win=(3, 5))
PHYS_NOISE = 300.0                                       # against the speckle's 1000: the static half decorrelates by noise alone
PHYS_STATIC, PHYS_MOVING = slice(16, 112), slice(144, 240)   # the halves away from their boundary: the split gives up axial resolution
# What the model shows on this field (tests/test_ssada_cases.py prints and asserts it): the moving half's median decorrelation is
# 4.2 (1 band) and 4.7 (4 bands) times the static half's, and the static half's spread with 4 bands 0.42 of its spread with 1.
PHYS_MEDIAN_MARGIN, PHYS_SPREAD_MARGIN = 2.0, 0.75


@functools.lru_cache(maxsize=None)
def physics_field():
    """1 group x 4 repeats of 16 A-scans x 256 points: static on depths < 128, independent beyond, with noise of PHYS_NOISE."""
    rng = np.random.default_rng(1077)
    X = ac.field(1, 4, 16, 256, 77, kind="vessel")
    X = (X + (rng.normal(0, PHYS_NOISE, X.shape) + 1j * rng.normal(0, PHYS_NOISE, X.shape)) / np.sqrt(2.0)).astype(np.complex64)
    X.setflags(write=False)
    return X


def physics_check(decorr_by_bands, what):
    """The ordering, on {1: decorr, 4: decorr} of physics_field() (each (1, 16, 256)); prints first."""
    spread = {}
    for M in (1, 4):
        d = np.asarray(decorr_by_bands[M])[0]
        static, moving = d[:, PHYS_STATIC], d[:, PHYS_MOVING]
        spread[M] = float(static.std())
        print("%s, %d band(s): median decorr static %.4f, moving %.4f; static spread %.4f" % (what, M, np.median(static), np.median(moving), spread[M]))
        assert np.median(moving) > PHYS_MEDIAN_MARGIN * np.median(static) > 0, (what, M)
    assert spread[4] < PHYS_SPREAD_MARGIN * spread[1], (what, spread)


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
def resident(cus):
    """resident_blocks(CUs, 32 waves per CU, 256): the cap of the split and mean kernels' grids."""
    return cus * BLOCKS_PER_CU


def group_share(repeats, bands, ascans, dc):
    """A group's bytes of the workspace: the band pairs, d and p."""
    return bands * ascans * dc * (8 * repeats + 8)


def plan(nframes, repeats, bands, ascans, N, depth=(0, 0), max_workspace_bytes=0, cus=PLAN_CUS):
    """fdoct_ssada_plan's figures (for a call the library accepts)."""
    _, _, _, _, dc = sm.resolve(N, bands, 1.0, (0, 0), depth)
    groups = nframes // repeats
    share = group_share(repeats, bands, ascans, dc)
    cap = max_workspace_bytes if max_workspace_bytes else DEFAULT_WORKSPACE
    gpp = min(groups, cap // share)
    return dict(groups=groups, depth_count=dc, groups_per_pass=gpp, passes=-(-groups // gpp), lds_bytes=3 * N * 8,
                workgroups=min(gpp * repeats * ascans, resident(cus)), workspace_bytes=gpp * share)


def beyond(items, stride):
    """At least one and a half passes of `stride` items, the last one partial."""
    return 2 * items >= 3 * stride and items % stride != 0


def grid_ascans(cus, dc):
    """A-scans of the capped-grid case (one group of 2 repeats, depths dc): the split kernel's items (2 a A-scan) and the mean
    kernel's pixels (dc a A-scan, 256 a workgroup) both run at least one and a half passes, the last partial."""
    split_stride, mean_stride = resident(cus), resident(cus) * BLOCK
    H = max(-(-3 * split_stride // 4), -(-3 * mean_stride // (2 * dc))) + 1
    while not (beyond(2 * H, split_stride) and beyond(H * dc, mean_stride)):
        H += 1
    return H
