"""CPU checks of tests/stage_grid_sizes.py: for several CU counts every case of tests/test_gpu_stage_grids.py lies beyond the
cap of the grid it is meant to overrun, and the lowpass widths give the (f, G, staged) the GPU tests count on."""
import pytest

import stage_grid_sizes as s

CUS = [64, 104, 256, 304]


@pytest.mark.parametrize("cus", CUS)
def test_resident_is_four_workgroups_per_cu(cus):
    assert s.resident(cus) == 4 * cus and s.roi_waves(cus) == 16 * cus and s.capture_stride(cus) == 1024 * cus


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("dt", list(s.CAPTURE_RUN))
def test_capture_frames_take_one_and_a_half_strides_and_a_partial_workgroup(cus, dt):
    H, W, runs = s.capture_shape(dt, cus)
    V = s.CAPTURE_RUN[dt]
    assert W % V == s.CAPTURE_TAIL[dt] and 0 < W % V < V and -(-W // V) == 126 and runs == H * 126
    assert s.beyond(runs, s.capture_stride(cus)) and runs % s.BLOCK != 0
    assert runs < 2 * s.capture_stride(cus)            # ... and no larger than that takes
    assert (H - 2) * 126 * 2 < 3 * s.capture_stride(cus)
    if cus == 256:
        assert 3121 <= H <= 3123


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("dt", ["u16", "f64", "u8"])
def test_minmax_cases(cus, dt):
    H, W, nblk = s.minmax_one_frame(dt, cus)
    runs = H * 126
    assert nblk == min(-(-runs // 256), s.resident(cus))
    assert s.beyond(nblk, 64)                                        # the fold's lane loop: 64 partials a stride
    run = s.BLOCK * (nblk - 2) + 17                                  # where the GPU test plants the minimum
    assert run < runs and s.minmax_owner(run, nblk) == nblk - 2 >= 64
    n = s.minmax_many_frames(cus)
    assert n > s.resident(cus) and s.minmax_blocks(8 * 3, n, cus) == 1
    assert -(-n // s.WAVES_PER_BLOCK) > 1 and n % s.WAVES_PER_BLOCK != 0    # fold workgroups, the last one partial
    assert n <= 65535                                                # frames ride in gridDim.y


def test_minmax_owner_walks_the_workgroups_in_turn():
    assert [s.minmax_owner(t, 99) for t in (0, 255, 256, 98 * 256, 99 * 256 - 1, 99 * 256)] == [0, 0, 1, 98, 98, 0]


@pytest.mark.parametrize("W", sorted(s.LOWPASS_EXPECT))
def test_lowpass_widths_give_the_listed_shapes(W):
    f, G, L, lds, staged = s.lowpass_shape(W)
    assert (f, G, staged) == s.LOWPASS_EXPECT[W]
    assert f == W // 10 and G * L >= W and L % 8 == 0
    if staged:
        assert lds == 8 * G * L + 16 * f * (G + 1) <= 65536
    if f > 256:
        assert G == 1                                                # the analysis loop's second stride: f * G > 256 threads


def test_lowpass_staging_ends_at_5849():
    assert s.lowpass_shape(5849)[3] == 65536 and s.lowpass_shape(5849)[4]
    assert not s.lowpass_shape(5850)[4]
    assert all(s.lowpass_shape(W)[4] for W in range(1, 5850)) and not any(s.lowpass_shape(W)[4] for W in range(5850, 6400))
    assert set(s.LOWPASS_BATCH_WIDTHS + s.LOWPASS_WIDTHS) <= set(s.LOWPASS_EXPECT)
    assert {s.lowpass_shape(W)[1] for W in (369, 400, 519, 850)} == {7, 6, 5, 3}
    assert [W for W in s.LOWPASS_WIDTHS if 2570 <= W <= 5849 and s.lowpass_shape(W)[0] > 256] == [2570, 2571, 4096, 5120, 5849]


@pytest.mark.parametrize("cus", CUS)
def test_lowpass_rows_beyond_the_grid(cus):
    assert s.beyond(s.lowpass_rows(cus), s.resident(cus))
    assert s.resident(cus) + 5 < s.lowpass_rows(cus)                 # the row filtered alone lies in the second stride


@pytest.mark.parametrize("cus", CUS + [96, 240, 105])
def test_binning_tiles_do_not_divide_the_grid(cus):
    tr, tc = s.bin_tiles(cus)
    assert s.resident(cus) % (tr * tc) != 0
    if cus in CUS:
        assert (tr, tc) == (3, 2)
    n = s.bin_images(cus)
    assert s.beyond(n * tr * tc, s.resident(cus))
    for upr, upc in ((1, 1), (2, 2), (3, 1), (1, 3)):
        for quad in (False, True):
            rows, cols = s.bin_output(cus, upr, upc, quad)
            assert rows % upr == 0 and cols % upc == 0 and (cols % 4 == 0) == quad
            assert -(-rows // 32) == tr and -(-cols // 128) == tc and rows % 32 and cols % 128
    assert s.bin_output(256, 1, 1) == (65, 129)


def test_colour_cases_beyond_8192_workgroups():
    assert s.COLOUR_STRIDE == 2097152
    assert s.beyond(s.colour_px_items(), s.COLOUR_STRIDE)
    # the 16-byte kernel's case is sized by its memory: one pass and a partial second one, 36 million pixels
    items = s.colour_vec_items()
    assert items > s.COLOUR_STRIDE + s.COLOUR_STRIDE // 16 and items % s.COLOUR_STRIDE != 0
    assert s.COLOUR_VEC_OUT[2] % 16 == 5


@pytest.mark.parametrize("cus", CUS)
def test_readout_cases(cus):
    H, waves = s.hold_ascans(cus), s.roi_waves(cus)
    for w, lane_loads in ((H, 3), (H, 12), (H, 9), (H - 2, 3), (H - 2, 10), (H - 2, 7)):   # whole image / one pixel in; quads or rows
        items, slices = s.hold_items(w, 3, lane_loads, cus)
        assert slices == 1 and items == w + 1 and waves < items < 2 * waves and items % waves >= 299
    assert H % 4 == 0                                                # the transposed layout's 16-byte path
    assert s.beyond(s.minmax_bscans(cus), waves)                     # a wave per B-scan
    assert s.beyond(s.mean_bscans(cus), s.resident(cus))             # a workgroup per B-scan
    D, Hm = s.MEAN_SHAPE
    assert 256 < s.MEAN_WIDTH < 512 and s.MEAN_WIDTH < Hm and D >= 3
