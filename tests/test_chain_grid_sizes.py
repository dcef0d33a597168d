"""CPU checks of tests/chain_grid_sizes.py: for several CU counts every case of tests/test_gpu_chain_grids.py lies beyond the pass,
the stride or the slice it is meant to overrun, its base batch lies within one, and the shapes take the kernel forms the GPU
tests name."""
import pytest

import chain_grid_sizes as s

CUS = [64, 104, 228, 256, 304]


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("H", [5, 7])
def test_tall_and_base_batches_of_the_workgroup_per_row_kernel(cus, H):
    G = s.tall_groups(H, cus)
    rows = G * H
    assert G >= s.BASE_GROUPS and s.generic_tall(rows, cus)
    assert 2 * rows >= 3 * s.GEN_MAX_PER_CU * cus
    for k in range(1, s.GEN_MAX_PER_CU + 1):
        assert rows > k * cus and rows % (k * cus) != 0            # a second pass, and a partial last one, whatever per_cu
    assert rows < 2 * s.GEN_MAX_PER_CU * cus                         # ... and no larger than that takes
    assert s.generic_base(s.BASE_GROUPS * H, cus) and not s.generic_base(rows, cus)
    if (cus, H) == (256, 7):
        assert (G, rows) == (330, 2310)


def test_shapes_take_the_four_forms_of_the_kernel():
    for what, W, M, N, D, A, H, threads, buffers in s.GENERIC_FORMS:
        assert D <= N // 2 and H in (5, 7)
        two = s.generic_lds(W, M, N, D, 2)
        if buffers == 1:                                             # two buffers do not fit a CU's LDS: one, every step in place
            assert two + 1024 > s.LDS_BYTES and s.generic_lds(W, M, N, D, 1) + 1024 <= s.LDS_BYTES
            assert s.generic_per_cu(s.generic_lds(W, M, N, D, 1)) == 1
        else:
            assert two + 1024 <= s.LDS_BYTES and s.generic_threads(two) == threads, what
            assert s.generic_per_cu(two) == {256: 6, 512: 2, 1024: 1}[threads]
    assert s.generic_lds(2048, 4, 8192, 1024) == 77824
    assert s.SMALL[1:7] == (100, 1, 256, 100, 2, 7)
    what, W, M, N, D, A, H = s.GENERIC_ZERO_PAD
    assert W % 2 == 1 and M > 1 and H == 7                           # an odd width: the zero-pad transforms at full length


def test_ticket_launches_go_round_the_words():
    assert s.GEN_TICKET_WORDS < s.TICKET_LAUNCHES <= 2 * s.GEN_TICKET_WORDS


def test_passes_in_front_of_the_chain():
    assert s.PASS == 524288
    base, tall = s.pre_elements(s.PRE_BASE_FRAMES), s.pre_elements(s.PRE_TALL_FRAMES)
    assert (base, tall) == (150000, 900000)
    assert base <= s.PASS and s.beyond(tall, s.PASS) and tall % s.PASS_BLOCK == 160
    assert s.PRE_TALL_FRAMES % s.PRE_BASE_FRAMES == 0 and s.PRE_PAD > 0


@pytest.mark.parametrize("dt", ["u16", "u8"])
def test_fast_min_max_places(dt):
    H, W, nv = s.MINMAX_FAST_H, s.MINMAX_FAST_W[dt], s.fast_vectors(dt)
    assert nv == {"u16": 513, "u8": 257}[dt] and nv % s.MINMAX_BLOCK == 1        # a last vector stride that holds one vector
    assert H == 2 * s.MINMAX_PARTS + 3                                            # two full row rounds and a ragged third
    places = s.fast_places(dt)
    assert len(places) == 5 and all(0 <= r < H and 0 <= c < W for r, c in places)
    strides = [(r // s.MINMAX_PARTS, s.fast_vector_of(dt, c) // s.MINMAX_BLOCK) for r, c in places]
    last = (nv - 1) // s.MINMAX_BLOCK
    assert strides[0] == (0, 0) and strides[1] == (2, last) and strides[3] == (1, 0) and strides[4] == (2, last)
    if dt == "u16":
        assert strides[2] == (0, 1) and places[2][1] * 2 == s.MINMAX_BLOCK * s.VEC_BYTES   # the second stride's first sample
        assert last == 2 and s.fast_vector_of(dt, places[4][1]) == nv - 1
    n = len(places)
    assert all(places[k][0] != places[(k + 1) % n][0] for k in range(n))        # maximum and minimum never share a row


def test_slow_min_max_places():
    W, H = s.MINMAX_SLOW
    assert (W * 2) % s.VEC_BYTES != 0 and (W * 1) % s.VEC_BYTES != 0             # minmax_fast_kernel refuses the width
    (r0, c0), (r1, c1) = s.MINMAX_SLOW_AT
    assert r0 != r1 and r0 == H - 1 and c0 == W - 1
    assert c0 // s.MINMAX_THREADS == 2 and W - 2 * s.MINMAX_THREADS == 2        # the ragged third stride
    assert c1 == s.MINMAX_THREADS                                                # the first sample of the second
    assert s.MINMAX_DARK[0] * 2 % s.VEC_BYTES == 0                               # (only the dark frame keeps this one off the fast kernel)


@pytest.mark.parametrize("cus", CUS)
def test_more_frames_than_a_launch_holds(cus):
    n, (W, H, N, D) = s.MANY_FRAMES, s.MANY_SHAPE
    assert s.SLICE < n < 2 * s.SLICE and n % s.BASE_GROUPS != 0
    assert -(-n // s.FINISH_BLOCK) == 257 and n % s.FINISH_BLOCK != 0
    rows = n * H
    assert s.generic_tall(rows, cus) and s.generic_base(s.BASE_GROUPS * H, cus)
    if cus == 256:
        assert rows // (s.GEN_MAX_PER_CU * cus) == 170
    assert (W * 2) % s.VEC_BYTES == 0                                            # minmax_fast_kernel takes the frames
    assert s.generic_per_cu(s.generic_lds(W, 1, N, D)) == s.GEN_MAX_PER_CU
    assert s.transpose_wide(H, D) and not s.transpose_wide(H, s.MANY_D_NARROW)
    assert n * H * W * 2 < 40 << 20 and n * H * D * 4 < 40 << 20


def test_transpose_edges():
    (h0, d0, o0), (h1, d1, o1), (h2, d2, o2) = s.TRANSPOSE_EDGES
    assert not s.transpose_wide(h0, d0) and h0 % 32 and d0 % 32 and h0 % 4 and d0 % 4 and h0 > 32 and d0 > 64
    assert s.transpose_wide(h1, d1, o1 % 4 == 0) and h1 // 64 == 1 and h1 % 64 and d1 < 64
    assert (h2, d2) == (h1, d1) and not s.transpose_wide(h2, d2, o2 % 4 == 0)
