"""GPU tests of include/fdoct_calibrate.h -- the device-side normalisations, BscanDark's three captures held on the device and their
composition -- against tests/calibrate_model.py and against the existing host-side path, fdoct_capture_reference with
FDOCT_REF_NONE, which is the yardstick of every capture.  Every comparison is bit for bit on the doubles (as uint64 words) or on
the chain's floats (as uint32 words); there is no tolerance anywhere."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import calibrate_model as cm
import calibrate_sizes as cs
from calibrate_model import bits
from capture_model import DARK as REF_DARK, BACKGROUND as REF_BACKGROUND, NONE as REF_NONE
from fdoct_amd import Config, FdoctError, Reconstructor, capi, io
from fdoct_amd.capi import CAL_DARK, CAL_REFERENCE, CAL_SAMPLE
from test_gpu_capture import DTYPES, _DeviceFrames, _frames, _host_view
from test_gpu_lowpass import _DeviceRows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(width=32, height=6, numfftpoints=256, numdisplaypoints=128)      # the captures' 6 x 32 frames
GOLD = dict(width=128, height=96, numfftpoints=1024, numdisplaypoints=512)    # where the chain runs behind the calibration
LIMITS = [(0.0001, 1.0), (1.0, 0.0001)]                                       # the capture's, and lo > hi


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), what


def _same_f32(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(**SMALL))
    yield r
    r.close()


# ---- fdoct_normalize_rows_minmax -------------------------------------------------------------------------------------------------
def _device_ways(rec, x, lo, hi, per_row, pad):
    """Device memory in place (packed) and out of place (rows `pad` doubles apart, the padding poisoned: _DeviceRows.host checks
    that it came back untouched)."""
    rows, W = x.shape
    d = _DeviceRows(x)
    rec.normalize_rows_minmax_device(d.ptr, rows, W, 0, lo, hi, per_row)
    rec.synchronize()
    yield "device, packed, in place", d.host()
    src, dst = _DeviceRows(x, pad=pad), _DeviceRows(np.zeros_like(x), pad=pad)
    rec.normalize_rows_minmax_device(src.ptr, rows, W, src.pitch, lo, hi, per_row, dst.ptr)
    rec.synchronize()
    _same(src.host(), x, "the input of an out-of-place call changed")
    yield "device, padded by %d, out of place" % pad, dst.host()


def _every_way(rec, x, lo, hi, per_row):
    """The same rows through every door: device memory as above (two paddings: between them every width meets rows that are 16-byte
    aligned and rows that are not), padded device rows in place, host memory out of place (packed) and in place (padded rows)."""
    rows, W = x.shape
    yield from _device_ways(rec, x, lo, hi, per_row, pad=3)
    yield from itertools.islice(_device_ways(rec, x, lo, hi, per_row, pad=1), 1, None)
    d = _DeviceRows(x, pad=5)
    rec.normalize_rows_minmax_device(d.ptr, rows, W, d.pitch, lo, hi, per_row)
    rec.synchronize()
    yield "device, padded, in place", d.host()
    keep = x.copy()
    got = rec.normalize_rows_minmax(keep, lo, hi, per_row)
    _same(keep, x, "the input of an out-of-place call changed")
    yield "host, packed, out of place", got
    padded = np.full((rows, W + 5), -3.0)
    view = padded[:, :W]
    view[:] = x
    rec.normalize_rows_minmax(view, lo, hi, per_row, out=view)
    assert np.all(padded[:, W:] == -3.0)
    yield "host, padded, in place", view.copy()


def _check_every_way(rec, x, what):
    for (lo, hi), per_row in itertools.product(LIMITS, (False, True)):
        want = cm.normalize_rows_minmax(x, lo, hi, per_row)
        for way, got in _every_way(rec, x, lo, hi, per_row):
            _same(got, want, "%s, limits %g .. %g, per_row %d, %s" % (what, lo, hi, per_row, way))
    return want


@pytest.mark.parametrize("rows,width", [(3, 8), (5, 24), (1, 1), (7, 161)])
def test_normalize_is_the_model_bit_for_bit(rec, rows, width):
    x = cm.plane(rows, width, seed=rows * 1000 + width)
    _check_every_way(rec, x, "%d x %d" % (rows, width))
    # ... and the library's own host helper, which the header names as the arithmetic
    _same(rec.normalize_rows_minmax(x, 0.0001, 1.0, per_row=False), capi.normalize_minmax(x.ravel(), 0.0001, 1.0).reshape(x.shape))
    _same(rec.normalize_rows_minmax(x, 0.0001, 1.0, per_row=True), np.stack([capi.normalize_minmax(r, 0.0001, 1.0) for r in x]))
    _same(rec.normalize_rows_minmax(x[0], -2.5, 17.0), capi.normalize_minmax(x[0], -2.5, 17.0), "one row as a 1-D array")


def test_normalize_constant_row_yields_shift(rec):
    x = cm.constant_row_plane()
    assert x[1].max() - x[1].min() <= cm.EPS
    _check_every_way(rec, x, "constant row")
    for lo, hi in LIMITS:
        got = rec.normalize_rows_minmax(x, lo, hi, per_row=True)
        assert np.all(got[1] == min(lo, hi)) and len(np.unique(got[0])) > 1
    flat = np.full((4, 9), 77.25)
    assert np.all(rec.normalize_rows_minmax(flat, 0.0001, 1.0, per_row=False) == 0.0001)     # a constant plane


def test_normalize_rounds_the_product_before_the_sum(rec):
    """On this plane a fused y * scale + shift differs from the separately rounded one in some element, per row and per plane
    (tests/test_calibrate_model.py); the host helper rounds twice, and so must the kernel."""
    x = cm.no_contraction_plane()
    _check_every_way(rec, x, "no-contraction plane")
    for per_row in (False, True):
        got = rec.normalize_rows_minmax(x, 0.0001, 1.0, per_row)
        fused = 0
        for r, row in enumerate(x):
            src = row if per_row else x
            scale, shift = cm.coefficients(float(src.min()), float(src.max()), 0.0001, 1.0)
            fused += sum(cm.fused(v, scale, shift) != got[r, c] for c, v in enumerate(row))
        assert fused >= 1


def test_normalize_host_to_device_and_back(rec):
    """One side in host memory, the other on the device, rows 3 doubles apart on both (the call has one pitch)."""
    x = cm.plane(5, 24, seed=11)
    want = cm.normalize_rows_minmax(x, 0.0001, 1.0, True)
    padded = np.full((5, 27), -3.0)
    padded[:, :24] = x
    dst = _DeviceRows(np.zeros_like(x), pad=3)
    rec._check(rec.lib.fdoct_normalize_rows_minmax(rec.h, padded.ctypes.data, capi.MEM_HOST, 5, 24, dst.pitch, 0.0001, 1.0, 1, dst.ptr,
                                                   capi.MEM_DEVICE))
    rec.synchronize()
    _same(dst.host(), want, "host rows to device rows")
    src = _DeviceRows(x, pad=3)
    out = np.full((5, 27), -7.0)
    rec._check(rec.lib.fdoct_normalize_rows_minmax(rec.h, src.ptr, capi.MEM_DEVICE, 5, 24, src.pitch, 0.0001, 1.0, 1, out.ctypes.data,
                                                   capi.MEM_HOST))
    _same(out[:, :24], want, "device rows to host rows")
    assert np.all(out[:, 24:] == -7.0) and np.all(padded[:, 24:] == -3.0)
    _same(src.host(), x)


@pytest.mark.parametrize("per_row", [True, False])
def test_normalize_tall_thin_plane_beyond_one_pass(rec, per_row):
    """More rows of 4 doubles than the capped grid has teams (pass 1), threads (pass 2: one a row) and half its threads (the scale
    pass: two runs a row); as one plane its extremes lie in the last pass of the reduction."""
    cus = _cus()
    H, W = cs.tall_thin(cus)
    s = cs.minmax_shape(H, W, per_row, cus)
    assert cs.beyond(2 * H, cs.lanes(cus))
    if per_row:
        assert s["T"] == 2 and s["S"] == 1 and cs.beyond(H, s["teams"]) and cs.beyond(H, cs.lanes(cus))
        x = cm.rows_extremes_plane(H, W, seed=4)
    else:
        min_at, max_at = cs.extreme_positions(H, W)
        last = cs.last_pass_start(s["items"], s["step"])
        assert last > 0 and cs.run_of(*min_at, W) >= last and cs.run_of(*max_at, W) >= last
        x = cm.extremes_plane(H, W, 4, min_at, max_at)
    want = cm.normalize_rows_minmax(x, 0.0001, 1.0, per_row)
    assert abs(want.min() - 0.0001) < 1e-12 and abs(want.max() - 1.0) < 1e-12   # (the limits, to the rounding of two operations)
    for way, got in _device_ways(rec, x, 0.0001, 1.0, per_row, pad=1):
        _same(got, want, way)


@pytest.mark.parametrize("per_row", [True, False])
def test_normalize_wide_plane_beyond_one_pass(rec, per_row):
    """Three rows of more runs than one and a half passes of the scale pass's grid take; every lane of the reduction loads in
    several passes and pass 2 strides over more partials than a team has lanes; the extremes lie in the last pass.  The width is
    odd: packed rows alternate in alignment (sample by sample), rows padded by one double are 16-byte aligned."""
    cus = _cus()
    H, W = cs.wide(cus)
    s = cs.minmax_shape(H, W, per_row, cus)
    assert cs.beyond(H * -(-W // 2), cs.lanes(cus)) and s["S"] > 64 and 2 * s["items"] >= 3 * s["step"]
    last = cs.last_pass_start(s["items"], s["step"])
    if per_row:
        assert cs.run_of(0, W - 3, W) >= last > 0
        x = cm.rows_extremes_plane(H, W, seed=5)
    else:
        min_at, max_at = cs.extreme_positions(H, W)
        assert last > 0 and cs.run_of(*min_at, W) >= last and cs.run_of(*max_at, W) >= last
        x = cm.extremes_plane(H, W, 5, min_at, max_at)
    want = cm.normalize_rows_minmax(x, 0.0001, 1.0, per_row)
    assert abs(want.min() - 0.0001) < 1e-12 and abs(want.max() - 1.0) < 1e-12   # (the limits, to the rounding of two operations)
    for way, got in _device_ways(rec, x, 0.0001, 1.0, per_row, pad=1):
        _same(got, want, way)


# ---- fdoct_calibrate_capture -----------------------------------------------------------------------------------------------------
def _capture_cases():
    """dtype x (donotnormalize, rowwisenormalize) x movavgn in full; host / device frames, nframes and raw-accumulate are laid over
    that product so that every value of any one option meets every value of any other (checked: a pairing that ties two options
    together would hide a path)."""
    flags, movs = [(1, 0), (0, 0), (1, 1), (0, 1)], [0, 2]
    rows = []
    for (di, dt), (fi, (dnn, rwn)), (mi, mov) in itertools.product(enumerate(DTYPES), enumerate(flags), enumerate(movs)):
        rows.append((dt, dnn, rwn, mov, (di + fi + mi) % 2, (1, 3)[(di + fi // 2 + mi) % 2], (di // 2 + fi + mi) % 2))
    options = [lambda r: r[0], lambda r: (r[1], r[2]), lambda r: r[3], lambda r: r[4], lambda r: r[5], lambda r: r[6]]
    for a, b in itertools.combinations(options, 2):
        seen = {(a(r), b(r)) for r in rows}
        assert len(seen) == len({a(r) for r in rows}) * len({b(r) for r in rows}), "two options of the matrix are tied together"
    return [pytest.param(*r, id="%s-dnn%d-rwn%d-mov%d-%s-n%d-raw%d" % (r[0], r[1], r[2], r[3], "dev" if r[4] else "host", r[5], r[6]))
            for r in rows]


def _calibrate(rec, slot, frames, device, out=True, pad=0):
    if device:
        d = _DeviceFrames(frames, pad)
        return rec.calibrate_capture_device(slot, d.ptr, d.dtype, d.n, d.pitch, out=out)
    return rec.calibrate_capture(slot, _host_view(frames, pad) if pad else frames, out=out)


@pytest.mark.parametrize("dt,dnn,rwn,mov,device,nframes,raw", _capture_cases())
def test_capture_equals_the_host_side_path_and_the_model(dt, dnn, rwn, mov, device, nframes, raw):
    W, H = SMALL["width"], SMALL["height"]
    r = Reconstructor(Config(rowwisenormalize=rwn, donotnormalize=dnn, movavgn=mov, **SMALL))
    frames = _frames(DTYPES[dt], nframes, H, W, seed=300 + nframes)
    recipe = dict(rowwisenormalize=rwn, donotnormalize=dnn, movavgn=0 if raw else mov)
    for lowpass in (False, True):
        r.set_capture_options(lowpass=lowpass, raw_accumulate=raw)
        yard = r.capture_reference(REF_NONE, frames, out=True)                  # the existing host-side path
        for slot in (CAL_REFERENCE, CAL_SAMPLE, CAL_DARK):
            got = _calibrate(r, slot, frames, device, pad=slot)                  # (padded rows for two of the three)
            _same(got, yard, "slot %d, lowpass %d" % (slot, lowpass))
        if not lowpass:
            _same(got, cm.capture(frames, **recipe), "the model")
        _same(r.get_reference(REF_DARK), yard, "the dark slot is the handle's dark frame")
        assert r.get_reference(REF_BACKGROUND) is None and r.calibrate_state() == (True, True, True)
    r.close()


@pytest.mark.parametrize("device", [False, True])
def test_capture_behind_a_2x2_front_end_on_u8(device):
    W, H = SMALL["width"], SMALL["height"]
    kw = dict(rowwisenormalize=1, donotnormalize=0, movavgn=2)
    r = Reconstructor(Config(**SMALL, **kw))
    r.set_frontend(0, 2, 2)
    raw = _frames(np.uint8, 3, 2 * H, 2 * W, seed=8)
    yard = r.capture_reference(REF_NONE, raw, out=True)
    got = _calibrate(r, CAL_SAMPLE, raw, device, pad=3)
    _same(got, yard, "behind the front end")
    _same(got, cm.capture(raw, binx=2, biny=2, **kw), "the model")
    r.set_frontend(3, 2, 2)                                                     # ... and with the median in front of the binning
    _same(_calibrate(r, CAL_REFERENCE, raw, device), r.capture_reference(REF_NONE, raw, out=True), "median 3")
    _same(_calibrate(r, CAL_REFERENCE, raw, device), cm.capture(raw, mediann=3, binx=2, biny=2, **kw), "median 3, the model")
    assert r.calibrate_state() == (False, True, True)
    r.close()


# ---- fdoct_calibrate_compose, the slots, the dark frame ---------------------------------------------------------------------------
def _three(H, W, seed, n=3):
    """Dark, reference-arm and sample-arm frames: the dark a fraction of the arms, so that the composed background is positive."""
    f = _frames(np.uint16, 3 * n, H, W, seed).reshape(3, n, H, W)
    return (f[0] // 16).astype(np.uint16), f[1], f[2]


def _host_recipe(r, dark, ref, smp, dark_role=REF_NONE):
    """INTEGRATION.md 2d before this stage existed: three captures to the host, the loop, the background setter."""
    yd = r.capture_reference(dark_role, dark, out=True)
    yr = r.capture_reference(REF_NONE, ref, out=True)
    ys = r.capture_reference(REF_NONE, smp, out=True)
    yb = cm.host_loop(yr, ys, yd)
    r.set_background(yb)
    return yb


@pytest.mark.parametrize("lowpass", [False, True])
@pytest.mark.parametrize("dnn,rwn", [(1, 0), (0, 1)])
def test_compose_equals_the_host_loop_and_becomes_the_background(dnn, rwn, lowpass):
    W, H = SMALL["width"], SMALL["height"]
    r = Reconstructor(Config(rowwisenormalize=rwn, donotnormalize=dnn, movavgn=2, **SMALL))
    r.set_capture_options(lowpass=lowpass)
    dark, ref, smp = _three(H, W, seed=21)
    want = _host_recipe(r, dark, ref, smp)
    r.set_background(np.full(W, 5.0))                                            # something else, to be replaced
    assert r.calibrate_state() == (False, False, False)
    _calibrate(r, CAL_DARK, dark, device=True, out=False)
    _calibrate(r, CAL_REFERENCE, ref, device=False, out=False)                   # (no download: the slot alone holds it)
    _calibrate(r, CAL_SAMPLE, smp, device=True, out=False, pad=2)
    got = r.calibrate_compose(out=True)
    _same(got, want, "the composition")
    yb = r.get_reference(REF_BACKGROUND)
    assert yb.shape == (H, W)                                                    # rows = H
    _same(yb, want, "fdoct_get_reference(BACKGROUND)")
    assert r.calibrate_state() == (True, True, True)                             # the slots stay held
    r.calibrate_compose()                                                        # ... so that it can be composed again, without out_host
    _same(r.get_reference(REF_BACKGROUND), want)
    r.close()


def test_process_after_the_calibration_equals_the_host_recipe():
    W, H = GOLD["width"], GOLD["height"]
    kw = dict(rowwisenormalize=0, donotnormalize=1, movavgn=0)
    dark, ref, smp = _three(H, W, seed=22)
    live = _frames(np.uint16, 2, H, W, seed=23)
    a, b = Reconstructor(Config(**GOLD, **kw)), Reconstructor(Config(**GOLD, **kw))
    for slot, f in ((CAL_DARK, dark), (CAL_REFERENCE, ref), (CAL_SAMPLE, smp)):
        _calibrate(a, slot, f, device=True, out=False)
    a.calibrate_compose()
    yb = _host_recipe(b, dark, ref, smp, dark_role=REF_DARK)                      # data_yd is in use as soon as it is captured
    assert yb.min() > 0
    _same(a.get_reference(REF_BACKGROUND), b.get_reference(REF_BACKGROUND))
    _same(a.get_reference(REF_DARK), b.get_reference(REF_DARK))
    (bs_a, db_a), (bs_b, db_b) = a.process(live), b.process(live)
    assert np.isfinite(bs_a).all()
    _same_f32(bs_a, bs_b, "bscan")
    _same_f32(db_a, db_b, "bscandb")
    a.close()
    b.close()


def test_dark_slot_is_the_dark_frame_the_chain_subtracts():
    W, H = GOLD["width"], GOLD["height"]
    kw = dict(rowwisenormalize=0, donotnormalize=1, movavgn=0)
    dark, ref, _ = _three(H, W, seed=24)
    live = _frames(np.uint16, 2, H, W, seed=25)
    a, b, c = (Reconstructor(Config(**GOLD, **kw)) for _ in range(3))
    yb = ref.sum(axis=0, dtype=np.float64) / len(ref)
    for r in (a, b, c):
        r.set_background(yb)
    got = _calibrate(a, CAL_DARK, dark, device=True)
    want = b.capture_reference(REF_DARK, dark, out=True)
    _same(got, want)
    _same(a.get_reference(REF_DARK), want, "fdoct_get_reference(DARK) equals the slot")
    assert a.calibrate_state() == (True, False, False)
    (bs_a, _), (bs_b, _), (bs_c, _) = a.process(live), b.process(live), c.process(live)
    _same_f32(bs_a, bs_b, "a handle that used FDOCT_REF_DARK")
    assert not np.array_equal(bs_a, bs_c)                                        # ... and the dark frame is subtracted at all
    a.calibrate_clear()                                                          # the slots go, the dark frame stays
    assert a.calibrate_state() == (False, False, False)
    _same(a.get_reference(REF_DARK), want)
    for r in (a, b, c):
        r.close()


def test_empty_slots_failed_captures_and_clear():
    W, H = SMALL["width"], SMALL["height"]
    r = Reconstructor(Config(**SMALL))
    dark, ref, smp = _three(H, W, seed=26)
    before = np.full((1, W), 5.0)
    r.set_background(before[0])
    out = np.full((H, W), -7.0)
    for held in ((), (CAL_DARK,), (CAL_DARK, CAL_SAMPLE)):                       # an empty slot: FDOCT_ERR_STATE, nothing changes
        for slot in held[-1:]:
            _calibrate(r, slot, (dark, ref, smp)[slot], device=False, out=False)
        assert r.lib.fdoct_calibrate_compose(r.h, out.ctypes.data) == -5 and "held" in r.lib.fdoct_last_error(r.h).decode()
        assert np.all(out == -7.0)
        _same(r.get_reference(REF_BACKGROUND), before, "the background after a refused composition")
    _calibrate(r, CAL_REFERENCE, ref, device=True, out=False)
    first = r.calibrate_compose(out=True)
    _same(first, cm.compose(*(cm.capture(f, donotnormalize=1) for f in (ref, smp, dark))))
    # a failed capture leaves the slot's previous content in place
    yd = r.get_reference(REF_DARK)
    with pytest.raises(FdoctError) as e:
        r.calibrate_capture(CAL_REFERENCE, np.zeros((2, H, W - 1), np.uint16))   # narrower frames: the pitch is smaller than a row
    assert e.value.code == -1
    assert r.lib.fdoct_calibrate_capture(r.h, CAL_DARK, smp.ctypes.data, capi.DTYPE_U16, capi.MEM_HOST, 0, 0, out.ctypes.data) == -1
    assert r.lib.fdoct_calibrate_capture(r.h, 3, smp.ctypes.data, capi.DTYPE_U16, capi.MEM_HOST, 3, 0, out.ctypes.data) == -1
    assert r.lib.fdoct_calibrate_capture(r.h, CAL_SAMPLE, smp.ctypes.data, 9, capi.MEM_HOST, 3, 0, out.ctypes.data) == -1
    assert np.all(out == -7.0) and r.calibrate_state() == (True, True, True)
    _same(r.get_reference(REF_DARK), yd)
    _same(r.calibrate_compose(out=True), first, "the slots after failed captures")
    # a new capture replaces one slot only
    _calibrate(r, CAL_SAMPLE, ref, device=True, out=False)
    _same(r.calibrate_compose(out=True), cm.compose(*(cm.capture(f, donotnormalize=1) for f in (ref, ref, dark))))
    # a clone starts with empty slots; clear empties them here
    twin = r.clone_to_device(0)
    assert twin.calibrate_state() == (False, False, False)
    _same(twin.get_reference(REF_DARK), yd)                                      # (the dark frame is set-up state and travels)
    twin.close()
    r.calibrate_clear()
    assert r.calibrate_state() == (False, False, False)
    assert r.lib.fdoct_calibrate_compose(r.h, None) == -5
    _same(r.get_reference(REF_DARK), yd)
    _calibrate(r, CAL_DARK, dark, device=True, out=False)                        # ... and they fill again
    assert r.calibrate_state() == (True, False, False)
    r.close()


def test_host_harness_calibrates_from_dark_reference_and_sample_frames(tmp_path):
    """host/bscanfft_sim --calibrate-dark-ref-sample 3: the C++ caller's composed background and B-scans against the Python path."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    exe = os.path.join(ROOT, "host", "bscanfft_sim")
    W, H, N, D = GOLD["width"], GOLD["height"], GOLD["numfftpoints"], GOLD["numdisplaypoints"]
    dark, ref, smp = _three(H, W, seed=27)
    live = _frames(np.uint16, 2, H, W, seed=28)
    f_ocv = str(tmp_path / "frames.ocv")
    io.write_ocv(f_ocv, np.concatenate([dark, ref, smp, live]).reshape(11 * H, W))
    prefix = str(tmp_path / "out")
    cmd = [exe, "--frames", f_ocv, "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N),
           "--numdisplaypoints", str(D), "--out", prefix, "--calibrate-dark-ref-sample", "3", "--capture-lowpass"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
    got = np.fromfile(prefix + "_background.f64", np.float64).reshape(H, W)
    bscan = np.fromfile(prefix + "_bscan.f32", np.float32).reshape(-1, D, H)
    assert bscan.shape[0] == 2
    r = Reconstructor(Config(**GOLD))
    r.set_capture_options(lowpass=True)
    want = _host_recipe(r, dark, ref, smp, dark_role=REF_DARK)
    _same(got, want, "bscanfft_sim's composed background")
    pb, _ = r.process(live, layout=capi.LAYOUT_TRANSPOSED)
    r.close()
    _same_f32(bscan, pb, "bscanfft_sim's B-scans")
