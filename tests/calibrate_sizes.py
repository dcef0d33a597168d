"""The case sizes of tests/test_gpu_calibrate.py as pure functions of the card's CU count, and the launch arithmetic of
fdoct_calibrate.hip restated next to them (minmax_shape and the capped grids), in the style of tests/stage_grid_sizes.py.
tests/test_calibrate_model.py holds every case to its condition on the CPU for several CU counts; the GPU tests assert the same
conditions on the card they run on.

The min / max of a group (a row, or the whole plane) is folded by TEAMS of T lanes, one SEGMENT of the group each: a team takes
runs seg * T + lane, + S * T, ... of its group (a run is 2 doubles), and the grid's teams take units (group, segment) in a
grid-stride loop.  The scale pass is a plain grid-stride loop over all runs."""
from stage_grid_sizes import BLOCK, beyond, resident

RUN = 2               # doubles a lane loads at once (CAL_RUN)
MIN_RUNS = 4          # CAL_MIN_RUNS
MAX_SEGMENTS = 4096   # CAL_MAX_SEGMENTS


def lanes(cus):
    """Threads of a capped grid: one pass of the scale kernel's loop takes this many runs."""
    return resident(cus) * BLOCK


def pow2_up_to_wave(n):
    t = 1
    while t < 64 and t < n:
        t <<= 1
    return t


def minmax_shape(rows, W, per_row, cus):
    """minmax_shape of fdoct_calibrate.hip as a dict: groups, items (runs per group), cpr, T, S, T2, teams (of the capped grid),
    units, step (runs between two loads of a lane), blocks, blocks2, ws_doubles."""
    cpr = -(-W // RUN)
    groups = rows if per_row else 1
    items = (1 if per_row else rows) * cpr
    T = pow2_up_to_wave(items)
    teams = lanes(cus) // T
    worth = -(-items // (MIN_RUNS * T))
    S = max(1, min(teams // groups, worth, MAX_SEGMENTS))
    T2 = pow2_up_to_wave(S)
    units = groups * S
    cap = resident(cus)
    return dict(groups=groups, items=items, cpr=cpr, T=T, S=S, T2=T2, teams=teams, units=units, step=S * T,
                blocks=max(1, min(-(-units * T // BLOCK), cap)), blocks2=max(1, min(-(-groups * T2 // BLOCK), cap)),
                ws_doubles=2 * units + 2 * groups)


TALL_W = 4            # two runs a row: teams of 2 lanes, 32 rows a wave


def tall_thin(cus):
    """(H, W) with more rows than pass 2 has threads (it folds a row's single partial with one thread): one and a half passes of
    its loop, the last partial.  That is three passes of the per-row reduction's unit loop (two lanes a row) and of the scale
    pass's runs (two a row)."""
    H = 3 * lanes(cus) // 2 + 3
    while H % lanes(cus) == 0 or H % (lanes(cus) // 2) == 0:
        H += 1
    return H, TALL_W


WIDE_H = 3


def wide(cus):
    """(H, W) of three rows whose runs exceed one and a half passes of the scale pass's grid; W is odd, so every row ends in a
    run of one double and no row but the first is 16-byte aligned when the rows are packed."""
    cpr = lanes(cus) // 2 + 2
    while (WIDE_H * cpr) % lanes(cus) == 0:
        cpr += 1
    return WIDE_H, RUN * cpr - 1


def last_pass_start(items, stride):
    """The first item of the last pass of a loop that takes `stride` items a pass."""
    return (items - 1) // stride * stride


def run_of(r, c, W):
    """The run (item of the scale pass and of the plane's reduction) that holds sample (r, c)."""
    return r * -(-W // RUN) + c // RUN


def extreme_positions(H, W):
    """(min_at, max_at) of the planes whose extremes lie at the very end: the last row's last column and two columns before it,
    two different runs, the last two of the plane."""
    return (H - 1, W - 1), (H - 1, W - 3)
