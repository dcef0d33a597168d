"""The case sizes of tests/test_gpu_chain_grids.py as pure functions of the card's CU count, and the launch arithmetic of the
reconstruction chain restated next to them: generic_kernel's grid and row tickets, the passes in front of the chain, the
whole-frame min / max pre-pass and the transpose pass.  tests/test_chain_grid_sizes.py holds every case to its condition on the
CPU for several CU counts; the GPU tests assert the same inequalities on the card they run on, so a later change of a constant
makes a test say so instead of passing one stride short.

Keep the figures equal to the launch code they are taken from:"""

PASS = 2048 * 256        # elements one pass of dim3(2048) x dim3(256) takes: movavg_f64_kernel<double>, <float>, movavg_kernel
#                          fdoct_generic.hip:670, :674, :680; f64_split_kernel fdoct_prepass_launch.inc:56
PASS_BLOCK = 256
MINMAX_PARTS = 16        # workgroups per frame of minmax_fast_kernel: rows r += 16                   fdoct_prepass_kernels.inc:40, :60
MINMAX_BLOCK = 256       # ... threads of each: 16-byte vectors v += 256                             fdoct_prepass_kernels.inc:62, fdoct_prepass_launch.inc:14
VEC_BYTES = 16
MINMAX_THREADS = 1024    # minmax_kernel: i += 1024                                                  fdoct_prepass_kernels.inc:13, fdoct_prepass_launch.inc:25
FINISH_BLOCK = 256       # frames per workgroup of minmax_finish_kernel                              fdoct_prepass_kernels.inc:93, fdoct_prepass_launch.inc:22
SLICE = 65535            # frames of one minmax_fast_kernel launch (gridDim.y), groups of one transpose launch (gridDim.z)
#                          fdoct_prepass_launch.inc:12, :40, :46
GEN_MAX_PER_CU = 6       # generic_kernel: grid = min(CUs x per_cu, out_rows), 1 <= per_cu <= 6       fdoct_route_value.cpp, make_route
GEN_TICKET_WORDS = 64    # row counters used in turn, gen_ticket_seq++ % 64                          fdoct_route.cpp, launch_family_generic
LDS_BYTES = 160 * 1024


def beyond(items, stride):
    """At least one and a half passes of `stride` items, the last one partial."""
    return 2 * items >= 3 * stride and items % stride != 0


# ---- generic_kernel: a workgroup's first row is its index, every further one a ticket (fdoct_generic.hip:254-262, :598) ---------
def generic_lds(W, M, N, D, buffers=2):
    """generic_lds_bytes (fdoct_plan.cpp) of a real row with numdisplaypoints <= numfftpoints / 2 whose transforms run at half
    length as Stockham passes: the row, the DFT buffer(s), the magnitude sums."""
    L = N // 2
    if M > 1:
        L = max(L, W * M // 2)
    return ((W + 3) & ~3) * 4 + L * 8 * buffers + ((D + 3) & ~3) * 4


def generic_per_cu(lds):
    """Workgroups per CU that the route's grid counts (fdoct_route_value.cpp, make_route)."""
    return max(1, min(GEN_MAX_PER_CU, (LDS_BYTES - 1024) // lds))


def generic_threads(lds):
    """launch_generic's choice among generic_kernel<256, 6>, <512, 2> and <1024, 1> (fdoct_generic.hip:637-644)."""
    per_cu = (LDS_BYTES - 1024) // lds
    return 256 if per_cu >= 3 else 512 if per_cu == 2 else 1024


def generic_tall(rows, cus):
    """The tests cannot see per_cu, so a tall batch is sized by its upper bound: one and a half passes of 6 workgroups per CU,
    and a partial last pass whatever per_cu the LDS allows."""
    return 2 * rows >= 3 * GEN_MAX_PER_CU * cus and all(rows % (k * cus) != 0 for k in range(1, GEN_MAX_PER_CU + 1))


def generic_base(rows, cus):
    """Every workgroup takes the row of its own index and nothing else."""
    return rows <= cus


def tall_groups(H, cus):
    """The fewest averaging groups of H rows that make a tall batch."""
    G = -(-3 * GEN_MAX_PER_CU * cus // (2 * H))
    while not generic_tall(G * H, cus):
        G += 1
    return G


BASE_GROUPS = 3
# (what, W, M, N, D, A, H, threads, DFT buffers): one shape per form of the kernel
GENERIC_FORMS = [
    ("256 x 6", 100, 1, 256, 100, 2, 7, 256, 2),
    ("512 x 2", 2048, 4, 8192, 1024, 2, 7, 512, 2),
    ("1024 x 1", 4096, 4, 16384, 2048, 2, 5, 1024, 2),
    ("1024 x 1 in place", 4096, 8, 32768, 2048, 1, 5, 1024, 1),
]
# a 161-column region of interest upsampled x4: zero-pad transforms of 161 and 643 points (a prime: Bluestein) at full length
# inside the kernel's LDS buffers (test_long_rows_and_any_zero_pad_length lists it for the family)
GENERIC_ZERO_PAD = ("full-length zero-pad, Bluestein", 161, 4, 2560, 320, 2, 7)
SMALL = GENERIC_FORMS[0]

TICKET_LAUNCHES = 70     # on one handle, none synchronised: 64 words and 6 reused


# ---- the passes in front of the chain: element loops of PASS ------------------------------------------------------------------
PRE_SHAPE = (1000, 50, 1024, 256)    # W, H, N, D; averages 1
PRE_BASE_FRAMES, PRE_TALL_FRAMES = 3, 18
PRE_PAD = 3                          # samples between the rows of the device frames


def pre_elements(frames):
    W, H = PRE_SHAPE[:2]
    return frames * H * W


# ---- the whole-frame min / max pre-pass -----------------------------------------------------------------------------------------
MINMAX_FAST_H = 35
MINMAX_FAST_W = {"u16": 4104, "u8": 4112}
# (row, column) of a frame's extreme: the first sample; the last one; the first sample of the 16-bit frames' second vector stride;
# the first row of the second row round; the last row, in the 16-bit frames' third vector stride and the 8-bit frames' second
MINMAX_FAST_AT = [(0, 0), (34, None), (15, 2048), (16, 7), (34, 4096)]


def fast_vectors(dt):
    es = {"u16": 2, "u8": 1}[dt]
    assert MINMAX_FAST_W[dt] * es % VEC_BYTES == 0
    return MINMAX_FAST_W[dt] * es // VEC_BYTES


def fast_vector_of(dt, col):
    return col * {"u16": 2, "u8": 1}[dt] // VEC_BYTES


def fast_places(dt):
    W = MINMAX_FAST_W[dt]
    return [(r, W - 1 if c is None else c) for r, c in MINMAX_FAST_AT]


MINMAX_SLOW = (2050, 3)              # W, H: rows that are not whole 16-byte vectors
MINMAX_SLOW_AT = [(2, 2049), (1, 1024)]
MINMAX_DARK = (2048, 3)

# ---- more frames than one launch's gridDim.y / gridDim.z holds --------------------------------------------------------------------
MANY_FRAMES = 65540
MANY_SHAPE = (64, 4, 128, 32)        # W, H, N, D
MANY_D_NARROW = 30                   # no multiple of 4: transpose_kernel


def transpose_wide(rows, cols, aligned=True):
    """launch_transpose takes transpose64_kernel (fdoct_prepass_launch.inc:39)."""
    return rows % 4 == 0 and cols % 4 == 0 and aligned


TRANSPOSE_EDGES = [(45, 67, 0), (68, 36, 0), (68, 36, 1)]   # H, D, floats the output pointers lie past a 16-byte boundary
