"""The fields and cases of the vibrometry stage's tests (tests/test_vibro_cases.py on the CPU, tests/test_gpu_vibro.py on the GPU),
and the launch arithmetic of the stage (fdoct_vibro_kernels.h) restated next to them, as pure functions: tests/test_vibro_cases.py
holds every case to its conditions on the CPU -- the exemption caps, |C| >= 16 tol_C with a reference, the double arithmetic's term,
the chunks a case is there for -- from tests/vibro_model.py alone.

Fields are generated directly as complex64, no chain in front: a seeded speckle amplitude per pixel that does not change over
time, a static phase per pixel, and over time a vibration a sin(2 pi nu0 t + psi) per pixel, a drift or a ramp, and a common-mode
phase per (frame, A-scan) that every depth shares; additive noise.  The bins of the reference surface are bright and carry the
common-mode phase only."""
import functools

import numpy as np

import vibro_model as vm
from vibro_model import HANN, RECT

# Keep equal to fdoct_vibro_kernels.h:
WAVES_PER_BLOCK = 4                 # kVibWaves
GRID_CAP = 1 << 16                  # kVibGridCap: the most workgroups of the reference and series passes
NU0 = 0.11                          # the fields' own vibration, cycles per frame


def field(T, H, D, seed, amax=1.2, drift=0.0, step=0.0, common=0.0, surface=None, zero_row=None, noise=4.0):
    """X (T, H, D) complex64.  amax: the largest vibration amplitude (rad); drift, step: rad per frame on every pixel; common: the
    half-width of the random common-mode phase per (frame, A-scan); surface: (first, count) of bright bins without vibration;
    zero_row: (frame, A-scan) that is exactly 0."""
    rng = np.random.default_rng(seed)
    amp = 900.0 * (0.35 + rng.rayleigh(0.8, (H, D)))
    static = rng.uniform(-np.pi, np.pi, (H, D))
    a, psi = rng.uniform(0.0, amax, (H, D)), rng.uniform(-np.pi, np.pi, (H, D))
    t = np.arange(T, dtype=np.float64)[:, None, None]
    phi = a[None] * np.sin(2 * np.pi * NU0 * t + psi[None]) + (drift + step) * t
    if surface:
        first, count = surface
        amp[:, first:first + count] = 2.0e4 * (1.0 + 0.1 * rng.uniform(-1, 1, (H, count)))
        static[:, first:first + count] = rng.uniform(-0.3, 0.3, (H, count))
        phi[:, :, first:first + count] = 0.0
    cm = rng.uniform(-common, common, (T, H, 1)) if common else 0.0
    X = amp[None] * np.exp(1j * (static[None] + phi + cm)) + (rng.normal(0, noise, (T, H, D)) + 1j * rng.normal(0, noise, (T, H, D)))
    X = X.astype(np.complex64)
    if zero_row is not None:
        X[zero_row[0], zero_row[1], :] = 0
    return X


def _case(what, T, H, D, seed, freq=(NU0,), ref=None, detrend=0, window=RECT, scale=1.0, min_power=0.0, chunk_steps=0, **fld):
    return dict(what=what, T=T, H=H, D=D, seed=seed, freq=tuple(freq), ref=ref, detrend=detrend, window=window, scale=scale,
                min_power=float(min_power), chunk_steps=chunk_steps, fld=fld)


EIGHT = (0.5, NU0, 0.03125, 0.25, 0.3333, 0.07, 0.41, 0.0123)   # nu = 0.5, whole and broken numbers of cycles

CASES = [
    # the shortest series
    _case("T 2, 1 x 1", 2, 1, 1, 1, freq=(0.5,)),
    _case("T 3, 1 x 1, Hann (w = 0 1 0)", 3, 1, 1, 2, freq=(0.5, 0.25), window=HANN),
    _case("T 2, 5 x 67, line (no residual)", 2, 5, 67, 3, freq=(0.5,), detrend=1),
    _case("T 3, 5 x 67", 3, 5, 67, 4, freq=(0.3,)),
    # wave tails and a second wave
    _case("T 5, 2 x 63", 5, 2, 63, 5), _case("T 5, 2 x 64", 5, 2, 64, 6), _case("T 5, 2 x 65", 5, 2, 65, 7), _case("T 5, 2 x 130", 5, 2, 130, 8),
    # chunks forced
    _case("T 8, 3 x 65, chunk 1", 8, 3, 65, 9, chunk_steps=1), _case("T 8, 3 x 65, chunk 2", 8, 3, 65, 9, chunk_steps=2),
    _case("T 8, 3 x 65, chunk 3, line, Hann", 8, 3, 65, 9, chunk_steps=3, detrend=1, window=HANN),
    _case("T 8, 3 x 65, chunk 7 (one chunk)", 8, 3, 65, 9, chunk_steps=7),
    _case("T 151, 2 x 130, chunk 50 (3 whole chunks)", 151, 2, 130, 10, chunk_steps=50, freq=(NU0, 0.02)),
    _case("T 152, 2 x 130, chunk 50 (a fourth of one step)", 152, 2, 130, 11, chunk_steps=50, detrend=1, drift=0.05),
    _case("T 150, 2 x 130, chunk 50 (the third one short)", 150, 2, 130, 12, chunk_steps=50, window=HANN),
    # the rule's own choice: four chunks; one
    _case("T 200, 2 x 130, the rule (4 chunks), reference", 200, 2, 130, 13, ref=(100, 6), surface=(100, 6), common=2.5, freq=(NU0, 0.5)),
    _case("T 20, 2 x 130, the rule (1 chunk)", 20, 2, 130, 14),
    # beyond one pass of the capped grids: 50001 x 2 pixels in 8 chunks, 9 x 50001 reference rows
    _case("T 9, 50001 x 2, chunk 1, reference (two passes of both grids)", 9, 50001, 2, 15, ref=(0, 1), chunk_steps=1, common=1.0, amax=0.8),
    # the reference range
    _case("T 12, 6 x 67, reference of one bin", 12, 6, 67, 16, ref=(20, 1), surface=(20, 1), common=3.0),
    _case("T 12, 6 x 67, reference over all depths", 12, 6, 67, 17, ref=True, surface=(30, 4), common=3.0),
    _case("T 12, 6 x 67, reference of the last bin, line", 12, 6, 67, 18, ref=(66, 0), surface=(66, 1), common=3.0, detrend=1),
    _case("T 6, 128 x 9, reference, a row of zeros", 6, 128, 9, 19, ref=(2, 3), surface=(2, 3), common=2.0, zero_row=(3, 77)),
    _case("T 40, 4 x 130, common mode of +-3 rad, reference", 40, 4, 130, 20, ref=(60, 8), surface=(60, 8), common=3.0),
    _case("T 40, 4 x 130, common mode of +-3 rad, no reference", 40, 4, 130, 20, surface=(60, 8), common=3.0),
    # unwrapping: 16 steps of 2.5 rad, 40 rad > 12 pi
    _case("T 17, 3 x 67, a ramp of 2.5 rad a frame", 17, 3, 67, 21, step=2.5, amax=0.2),
    _case("T 17, 3 x 67, the ramp under the line", 17, 3, 67, 21, step=2.5, amax=0.2, detrend=1, chunk_steps=5),
    # frequencies
    _case("T 64, 3 x 67, no frequency", 64, 3, 67, 22, freq=()),
    _case("T 64, 3 x 67, eight frequencies, Hann", 64, 3, 67, 23, freq=EIGHT, window=HANN),
    _case("T 64, 3 x 67, eight frequencies, chunk 16, line", 64, 3, 67, 24, freq=EIGHT, chunk_steps=16, detrend=1),
    # windows and detrends over a drift of 0.3 rad a frame
    _case("T 100, 2 x 67, drift 0.3, mean, rect", 100, 2, 67, 25, drift=0.3),
    _case("T 100, 2 x 67, drift 0.3, line, rect", 100, 2, 67, 25, drift=0.3, detrend=1),
    _case("T 100, 2 x 67, drift 0.3, line, Hann, chunk 33", 100, 2, 67, 25, drift=0.3, detrend=1, window=HANN, chunk_steps=33),
    # scale and mask
    _case("T 16, 3 x 67, scale -53.5", 16, 3, 67, 26, scale=-53.5, freq=(NU0, 0.5)),
    _case("T 16, 8 x 130, min_power", 16, 8, 130, 27, min_power=1.3e6),
    _case("T 16, 8 x 130, min_power, chunk 4, reference, scale -2", 16, 8, 130, 28, min_power=1.3e6, chunk_steps=4, ref=(10, 4), surface=(10, 4),
          common=1.5, scale=-2.0),
]


def case_field(c):
    return field(c["T"], c["H"], c["D"], c["seed"], **c["fld"])


def case_args(c):
    """The keywords of vibro_model's functions."""
    return dict(freq=c["freq"], ref=c["ref"], detrend=c["detrend"], window=c["window"], scale=c["scale"], min_power=c["min_power"],
                chunk_steps=c["chunk_steps"])


def case_params(c):
    """The keywords of fdoct_amd.vibrometry.params."""
    return case_args(c)


@functools.lru_cache(maxsize=None)
def case_refs(i):
    """(X, (model, truth, tolerances, exemptions)) of CASES[i]: computed once, shared, never written to."""
    c = CASES[i]
    X = case_field(c)
    kw = case_args(c)
    tol = vm.tolerances(X, **kw)
    refs = (vm.model(X, **kw), vm.model(X, truth=True, **kw), tol, vm.exemptions(X, tol=tol, **kw))
    X.setflags(write=False)
    return X, refs


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
def chunks(T, H, D, chunk_steps=0):
    return len(vm.chunks_of(T, chunk_steps if chunk_steps else vm.chunk_rule(T, H * D)))


def series_items(T, H, D, chunk_steps=0):
    """Workgroups' worth of work of the series pass (vibro_plan_launch: items)."""
    tiles = H * (-(-D // 64))
    return -(-tiles // WAVES_PER_BLOCK) * chunks(T, H, D, chunk_steps)


def ref_items(T, H):
    """... and of the reference pass: four (frame, A-scan) rows a workgroup."""
    return -(-(T * H) // WAVES_PER_BLOCK)


def beyond(items, stride):
    """At least one and a half passes of `stride` items, the last one partial."""
    return 2 * items >= 3 * stride and items % stride != 0
