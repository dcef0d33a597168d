"""The case sizes of tests/test_gpu_stage_grids.py as pure functions of the card's CU count, and the launch arithmetic of the
side-stage kernels restated next to them (fdoct_grid.h's resident_blocks, frame_minmax_blocks, lowpass_shape, bscanbin_plan's
tiles, blocks_for of fdoct_colour.hip, the three launchers of fdoct_roi.hip).  tests/test_stage_grid_sizes.py holds every case to
its condition on the CPU for several CU counts; the GPU tests assert the same inequalities on the card they run on, so a
later change of a constant makes a test say so instead of passing one stride short.

A grid-stride kernel's `stride` is the number of work items its capped grid takes in one pass.  Every case sized here holds
more than one pass; those the module sizes freely hold at least one and a half and end in a partial pass (`beyond`)."""

BLOCK = 256                 # threads of every side-stage workgroup
WAVES_PER_BLOCK = BLOCK // 64
COL_MAX_BLOCKS = 8192       # fdoct_colour.hip


def resident(cus):
    """resident_blocks(CUs, 16 waves per CU, 256): the cap of the capture, lowpass, binning and readout grids."""
    return cus * (16 // WAVES_PER_BLOCK)


def beyond(items, stride):
    """At least one and a half passes of the capped grid, the last one partial."""
    return 2 * items >= 3 * stride and items % stride != 0


# ---- 1. capture_accumulate_kernel: a thread owns a run of 16 bytes of one row ---------------------------------------------
CAPTURE_RUN = {"u8": 16, "u16": 8, "f32": 4, "f64": 2}   # samples per run
CAPTURE_WHOLE_RUNS = 125
CAPTURE_TAIL = {"u8": 7, "u16": 3, "f32": 1, "f64": 1}   # 0 < tail < run: the row ends in a run the 16-byte path does not take


def capture_stride(cus):
    return resident(cus) * BLOCK


def capture_shape(dt, cus):
    """(H, W, runs): rows of 125 whole runs and a tail, as few rows as give one and a half passes and a partial workgroup."""
    W = CAPTURE_WHOLE_RUNS * CAPTURE_RUN[dt] + CAPTURE_TAIL[dt]
    cpr = CAPTURE_WHOLE_RUNS + 1
    H = -(-3 * capture_stride(cus) // (2 * cpr)) + 1
    while (H * cpr) % BLOCK == 0 or (H * cpr) % capture_stride(cus) == 0:
        H += 1
    return H, W, H * cpr


# ---- 2. frame_minmax_kernel / frame_minmax_fold_kernel ------------------------------------------------------------------------
def minmax_blocks(runs, nframes, cus):
    """frame_minmax_blocks: partials per frame."""
    want = -(-runs // BLOCK)
    share = max(1, resident(cus) // max(1, nframes))
    return max(1, min(want, share))


MINMAX_ONE_ROWS = 200   # x 126 runs = 25200 runs: 99 workgroups wanted, one and a half strides of the fold's 64 lanes


def minmax_one_frame(dt, cus):
    """(H, W, nblk) of the single large frame: nblk > 64, so that the fold wave takes a second stride."""
    W = CAPTURE_WHOLE_RUNS * CAPTURE_RUN[dt] + CAPTURE_TAIL[dt]
    runs = MINMAX_ONE_ROWS * (CAPTURE_WHOLE_RUNS + 1)
    return MINMAX_ONE_ROWS, W, minmax_blocks(runs, 1, cus)


def minmax_owner(run, nblk):
    """The workgroup (of one frame's nblk) whose threads fold run `run`."""
    return (run // BLOCK) % nblk


def minmax_many_frames(cus):
    """More frames than resident workgroups: every frame's share is one workgroup."""
    return resident(cus) + 37


# ---- 3. lowpass_rows_kernel ---------------------------------------------------------------------------------------------
LP_T, LP_MAX_SLICES, LP_LDS_MAX = 8, 8, 64 * 1024


def lowpass_shape(W):
    """lowpass_shape's (f, G, L, lds bytes, staged) of a row of W doubles."""
    f = W // 10
    chunks = -(-W // LP_T)
    G = max(1, min(LP_MAX_SLICES, BLOCK // max(1, f), chunks))
    L = -(-chunks // G) * LP_T
    lds = 8 * G * L + 16 * f * (G + 1)
    staged = lds <= LP_LDS_MAX
    if not staged:
        G, L, lds = 1, chunks * LP_T, 0
    return f, G, L, lds, staged


def lowpass_rows(cus):
    r = resident(cus)
    return r + r // 2 + 3


LOWPASS_BATCH_WIDTHS = [128, 2570, 5850, 9, 1]
LOWPASS_WIDTHS = [369, 400, 519, 850, 2570, 2571, 4096, 5120, 5849, 5850, 5851]
# (f, G, staged) the widths above must give
LOWPASS_EXPECT = {128: (12, 8, True), 369: (36, 7, True), 400: (40, 6, True), 519: (51, 5, True), 850: (85, 3, True),
                  2570: (257, 1, True), 2571: (257, 1, True), 4096: (409, 1, True), 5120: (512, 1, True), 5849: (584, 1, True),
                  5850: (585, 1, False), 5851: (585, 1, False), 9: (0, 2, True), 1: (0, 1, True)}


# ---- 4. bscan_bin_kernel: a workgroup owns a tile of 32 x 128 outputs (memory rows x memory columns) --------------------------
BIN_TILE_R, BIN_TILE_C = 32, 128


def bin_tiles(cus):
    """(tiles_r, tiles_c) per image: 3 x 2 unless that count divides the grid, then the next shape that does not."""
    for tr, tc in ((3, 2), (3, 1), (5, 1), (7, 1), (11, 1)):
        if resident(cus) % (tr * tc) != 0:
            return tr, tc
    raise AssertionError("no tile shape for %d CUs" % cus)


def bin_output(cus, upr, upc, quad=False):
    """(memory rows, memory columns) of an output with bin_tiles(cus) tiles whose last tile of either direction is partial:
    the smallest multiples of the factors from one row past tiles_r - 1 tiles and one column past tiles_c - 1 tiles on whose
    column count is no multiple of 4 (quad: is one)."""
    tr, tc = bin_tiles(cus)
    rows = -(-((tr - 1) * BIN_TILE_R + 1) // upr) * upr
    cols = -(-((tc - 1) * BIN_TILE_C + 1) // upc) * upc
    while (cols % 4 == 0) != quad:
        cols += upc
    assert -(-rows // BIN_TILE_R) == tr and rows % BIN_TILE_R and -(-cols // BIN_TILE_C) == tc and cols % BIN_TILE_C
    return rows, cols


def bin_images(cus):
    """Images for one and a half passes of the tile loop and a partial one."""
    tr, tc = bin_tiles(cus)
    n = -(-3 * resident(cus) // (2 * tr * tc))
    while (n * tr * tc) % resident(cus) == 0:
        n += 1
    return n


# ---- 5. colour_px_kernel / colour_vec_kernel: 8192 workgroups -------------------------------------------------------------------
COLOUR_STRIDE = COL_MAX_BLOCKS * BLOCK   # output pixels (px) or groups of 16 output pixels (vec) in one pass
COLOUR_PX_OUT = (6, 600, 1000)           # frames, output rows, output columns: 3.6 million pixels
COLOUR_VEC_OUT = (18, 1000, 16 * 125 + 5)   # 2.25 million groups of 16 and a 5-column tail for colour_px_kernel


def colour_px_items():
    n, h, w = COLOUR_PX_OUT
    return n * h * w


def colour_vec_items():
    n, h, w = COLOUR_VEC_OUT
    return n * h * (w // 16)


# ---- 6. roi_hold_kernel, roi_minmax_kernel, roi_mean_kernel ---------------------------------------------------------------------
def roi_waves(cus):
    return resident(cus) * WAVES_PER_BLOCK


def hold_ascans(cus):
    return 16 * cus + 300


def hold_items(w, nb, lane_loads_per_bscan, cus):
    """Row-major roi_hold_kernel: (items, slices) of an ROI of w A-scans -- w + 1 runs in `slices` pieces."""
    per_slice = w + 1
    slices = max(1, roi_waves(cus) // per_slice)
    slices = min(slices, max(1, nb * lane_loads_per_bscan // 64 // 16))
    return per_slice * slices, slices


def minmax_bscans(cus):
    return 16 * cus + 16 * cus // 2 + 3


def mean_bscans(cus):
    r = resident(cus)
    return r + r // 2 + 3


MEAN_SHAPE = (5, 300)   # D x H
MEAN_WIDTH = 290        # two strides of the 256-thread column loop, the second partial
