"""The fields and cases of tests/test_gpu_doppler.py, and the launch arithmetic of the Doppler stage (fdoct_doppler_kernels.h)
restated next to them, as pure functions: tests/test_doppler_cases.py holds every case to its conditions on the CPU -- the
exemption caps, |B| >= 16 tol_B with the bulk correction, the tall batch's size for several CU counts -- from tests/doppler_model.py
alone.

Fields are generated directly as complex64, no chain in front: two reflectors on a decaying floor, additive noise, optionally
speckle; the phase of an A-scan is a static pattern along depth plus a ramp across A-scans and across frames, a flow region whose
ramp is steeper, and a small common offset per A-scan (the bulk motion).  The lag product's phase is therefore nearly the same at
every depth of a row -- the strong reflectors carry a common offset -- which is what keeps |B| well above its rounding error."""
import numpy as np

from doppler_model import ASCANS, FRAMES

# Keep equal to fdoct_boxtile.h and fdoct_doppler_kernels.h:
TILE_ROWS, TILE_DEPTHS = 16, 64     # kBoxRows, kBoxDepths
BLOCKS_PER_CU = 4                   # kBoxWavesPerCu / (kBoxBlock / 64): the cap of both kernels' grids, per CU
MAX_WIN = 32                        # kDopMaxWin


def field(n, H, D, seed, speckle=False, zero_row=None):
    """X (n, H, D) complex64.  zero_row: (frame, row) whose A-scan is exactly 0."""
    rng = np.random.default_rng(seed)
    b = np.arange(D, dtype=np.float64)
    amp = 800.0 * np.exp(-b / (D / 3.0 + 1.0)) + 2.0e4 * np.exp(-0.5 * ((b - 0.3 * D) / 1.5) ** 2) + 1.2e4 * np.exp(-0.5 * ((b - 0.7 * D) / 2.0) ** 2)
    static = rng.uniform(-np.pi, np.pi, D)
    flow = np.where((b > 0.4 * D) & (b < 0.6 * D), 0.9, 0.0)
    f, r = np.arange(n)[:, None, None], np.arange(H)[None, :, None]
    bulk = rng.uniform(-0.4, 0.4, (n, H, 1))
    phi = static[None, None, :] + 0.35 * r + 0.2 * f + flow[None, None, :] * (0.5 * r + 0.3 * f) + bulk
    a = amp[None, None, :] * np.ones((n, H, 1))
    if speckle:
        a = a * rng.rayleigh(0.8, (n, H, D))
    X = a * np.exp(1j * phi) + (rng.normal(0, 25.0, (n, H, D)) + 1j * rng.normal(0, 25.0, (n, H, D)))
    X = X.astype(np.complex64)
    if zero_row is not None:
        X[zero_row[0], zero_row[1], :] = 0
    return X


def _case(what, n, H, D, axis, lag, win, seed, bulk=None, min_power=0.0, scale=1.0, speckle=False, zero_row=None):
    return dict(what=what, n=n, H=H, D=D, axis=axis, lag=lag, win=win, seed=seed, bulk=bulk, min_power=float(np.float32(min_power)),
                scale=scale, speckle=speckle, zero_row=zero_row)


# Windows on both axes, depths of 1, 67, 130 (two tiles and two bins) and 320 (five tiles), pair rows below one tile (11, 12), of
# whole tiles (32) and of two and a half (39, 40), lags 1, 2 and the largest.
CASES = [
    _case("1 x 1, 2 x 12 x 67, A-scans lag 1", 2, 12, 67, ASCANS, 1, (1, 1), 1),
    _case("1 x 5, 2 x 12 x 67, A-scans lag 2", 2, 12, 67, ASCANS, 2, (1, 5), 2, speckle=True),
    _case("3 x 1, 3 x 17 x 130, frames lag 1", 3, 17, 130, FRAMES, 1, (3, 1), 3),
    _case("3 x 5, 2 x 40 x 320, A-scans lag 1, scale -2.5", 2, 40, 320, ASCANS, 1, (3, 5), 4, scale=-2.5, speckle=True),
    _case("4 x 8, 3 x 40 x 320, frames lag 1", 3, 40, 320, FRAMES, 1, (4, 8), 5),
    _case("32 x 32, 2 x 40 x 320, A-scans lag 1", 2, 40, 320, ASCANS, 1, (32, 32), 6, speckle=True),
    _case("32 x 32, 2 x 12 x 20, A-scans lag 1 (the window exceeds the image both ways)", 2, 12, 20, ASCANS, 1, (32, 32), 7),
    _case("3 x 5, 2 x 12 x 1, A-scans lag 1 (one depth)", 2, 12, 1, ASCANS, 1, (3, 5), 8),
    _case("4 x 8, 2 x 12 x 67, A-scans lag 11 (one pair row)", 2, 12, 67, ASCANS, 11, (4, 8), 9),
    _case("4 x 8, 3 x 33 x 130, A-scans lag 1 (32 pair rows)", 3, 33, 130, ASCANS, 1, (4, 8), 10, speckle=True),
    _case("3 x 5, 3 x 12 x 67, frames lag 2 (one pair image)", 3, 12, 67, FRAMES, 2, (3, 5), 11),
    # the bulk correction: every depth, a sub-range, a row of zeros (B = 0 exactly); the mask
    _case("3 x 5, 2 x 40 x 320, A-scans lag 1, bulk", 2, 40, 320, ASCANS, 1, (3, 5), 12, bulk=True, speckle=True),
    _case("4 x 8, 3 x 17 x 130, frames lag 1, bulk over depths 30..69", 3, 17, 130, FRAMES, 1, (4, 8), 13, bulk=(30, 40)),
    _case("1 x 1, 2 x 12 x 67, A-scans lag 1, bulk, a row of zeros", 2, 12, 67, ASCANS, 1, (1, 1), 14, bulk=True, zero_row=(1, 5)),
    _case("3 x 5, 2 x 12 x 67, A-scans lag 2, bulk from depth 20 on, a row of zeros", 2, 12, 67, ASCANS, 2, (3, 5), 15, bulk=(20, 0), zero_row=(0, 7)),
    _case("3 x 5, 2 x 40 x 320, A-scans lag 1, min_power", 2, 40, 320, ASCANS, 1, (3, 5), 16, min_power=1.0e5, speckle=True),
    _case("4 x 8, 3 x 17 x 130, frames lag 1, bulk, min_power, a row of zeros", 3, 17, 130, FRAMES, 1, (4, 8), 17, bulk=True, min_power=1.0e6,
          zero_row=(1, 3)),
]


def case_field(c):
    return field(c["n"], c["H"], c["D"], c["seed"], c["speckle"], c["zero_row"])


def case_args(c):
    """The keywords of doppler_model's functions and of Reconstructor.doppler alike."""
    return dict(axis=c["axis"], lag=c["lag"], win=c["win"], bulk=c["bulk"], scale=c["scale"], min_power=c["min_power"])


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
def tiles(pair_images, pair_rows, depths):
    """Tiles of doppler_kernel's loop (doppler_plan_launch)."""
    return pair_images * (-(-pair_rows // TILE_ROWS)) * (-(-depths // TILE_DEPTHS))


def grid_cap(cus):
    """resident_blocks(num_cu, kBoxWavesPerCu, kBoxBlock): the most workgroups either kernel is launched with."""
    return cus * BLOCKS_PER_CU


def beyond(items, stride):
    """At least one and a half passes of `stride` items, the last one partial."""
    return 2 * items >= 3 * stride and items % stride != 0


# The tall batch: frames of 13 A-scans x 67 depths.  A-scans, lag 1: 12 pair rows, two tiles a frame.  Frames, lag 3, on a base of
# six frames that holds three twice: three pair images, the tall batch's image p being the base's p mod 3.
TALL_H, TALL_D = 13, 67
TALL_BASE = {ASCANS: (3, 1), FRAMES: (6, 3)}   # axis: (base frames, lag)


def tall_frames(axis, cus):
    """The fewest frames whose tiles -- and, for the bulk kernel, pair rows -- go beyond one pass of the capped grid."""
    base_n, lag = TALL_BASE[axis]
    for n in range(base_n + 3, base_n + 3 + 3 * 100000, 3):
        if tall_ok(axis, n, cus):
            return n
    raise ValueError("no tall batch for %d CUs" % cus)


def tall_shape(axis, n):
    _, lag = TALL_BASE[axis]
    return (n - lag, TALL_H) if axis == FRAMES else (n, TALL_H - lag)


def tall_ok(axis, n, cus):
    pi, pr = tall_shape(axis, n)
    return n % 3 == 0 and beyond(tiles(pi, pr, TALL_D), grid_cap(cus)) and beyond(pi * pr, grid_cap(cus))


def base_ok(axis, cus):
    """The base batch lies within one pass: every workgroup takes at most one tile and one bulk row."""
    pi, pr = tall_shape(axis, TALL_BASE[axis][0])
    return tiles(pi, pr, TALL_D) <= grid_cap(cus) and pi * pr <= grid_cap(cus)
