"""GPU tests of include/fdoct_lowpass.h: BscanDark's lpfilter on rows of doubles (fdoct_lowpass_rows), as the last step of a
capture (fdoct_set_capture_options, lowpass) and the capture without the moving average (raw_accumulate), against
tests/lowpass_model.py and tests/capture_model.py.

The pass condition of every filtered result is the project's rule with the reference's float transform as the
allowance: tol = 1e-4 |truth| + 1e-6 max_row |truth|, and on EVERY element |gpu - truth| / tol <= max(0.5, |f32 model - truth|
/ tol).  Nothing is excluded.  What must be the same bits is compared as uint64 words."""
import os
import subprocess

import numpy as np
import pytest

import capture_model
import lowpass_model
from capture_model import BACKGROUND, DARK, NONE, PI, bits
from fdoct_amd import VARIANT_SIM, Config, Reconstructor, capi, io
from lowpass_model import lpfilter_truth
from test_gpu_capture import _DeviceFrames, _frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = dict(width=128, height=96, numfftpoints=1024, numdisplaypoints=512)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), what


def _holds(got, x, what, truth=None):
    worst, excess = lowpass_model.parity(got, x, truth)
    print("%s: worst |gpu - truth| / tol = %.3e" % (what, worst))
    assert excess <= 0, "%s: %.3e x tol, %.3e over the allowance" % (what, worst, excess)
    return worst


def _input(kind, rows, W, seed):
    if kind == "noise":
        return np.random.default_rng(seed).uniform(0.0001, 1.0, (rows, W))
    raw = _frames(np.uint16, 16, rows, W, seed).sum(axis=0, dtype=np.float64)   # what 16 accumulated camera frames hold
    return raw if kind == "sums" else capi.normalize_minmax(raw.ravel(), 0.0001, 1.0).reshape(rows, W)


class _DeviceRows:
    """(rows, W) doubles in device memory at a row pitch of `pad` doubles more than a row."""

    def __init__(self, x, pad=0):
        import torch
        rows, W = x.shape
        padded = np.full((rows, W + pad), -3.0)
        padded[:, :W] = x
        self.t = torch.from_numpy(padded).cuda()
        torch.cuda.synchronize()
        self.ptr, self.pitch, self.W = self.t.data_ptr(), (W + pad) * 8, W

    def host(self):
        import torch
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert np.all(a[:, self.W:] == -3.0), "the filter wrote into the padding"
        return a[:, :self.W]


def _every_way(rec, x):
    """The same rows through every door: device memory in place (packed) and out of place (padded), host memory out of place
    (packed) and in place (padded rows)."""
    rows, W = x.shape
    d = _DeviceRows(x)
    rec.lowpass_rows_device(d.ptr, rows, W)
    rec.synchronize()
    yield "device, packed, in place", d.host()
    src, dst = _DeviceRows(x, pad=3), _DeviceRows(np.zeros_like(x), pad=3)
    rec.lowpass_rows_device(src.ptr, rows, W, src.pitch, dst.ptr)
    rec.synchronize()
    _same(src.host(), x, "the input of an out-of-place call changed")
    yield "device, padded, out of place", dst.host()
    keep = x.copy()
    got = rec.lowpass_rows(keep)
    _same(keep, x, "the input of an out-of-place call changed")
    yield "host, packed, out of place", got
    padded = np.full((rows, W + 5), -3.0)
    view = padded[:, :W]
    view[:] = x
    rec.lowpass_rows(view, out=view)
    assert np.all(padded[:, W:] == -3.0)
    yield "host, padded, in place", view.copy()


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(**GEOM))
    yield r
    r.close()


@pytest.mark.parametrize("kind", ["sums", "normalised", "noise"])
@pytest.mark.parametrize("W", [9, 10, 128, 129, 130, 640, 1280, 2048, 2560])
@pytest.mark.parametrize("rows", [1, 96, 1000])
def test_lowpass_rows_meets_the_parity_rule_and_is_deterministic(rec, rows, W, kind):
    x = _input(kind, rows, W, seed=rows + W)
    truth = lpfilter_truth(x)
    first = None
    for what, got in _every_way(rec, x):
        if first is None:
            first = got
            _holds(got, x, "%d x %d %s, %s" % (rows, W, kind, what), truth)
            if W < 10:
                assert np.all(got == 0.0)
        else:   # the same bits at another pitch, from host memory, in place or not
            _same(got, first, what)
    again = rec.lowpass_rows(x)
    _same(again, first, "a second run")


@pytest.mark.parametrize("kind", ["normalised", "noise"])
def test_rows_too_long_for_lds(rec, kind):
    """24 000 doubles are 192 KB: the row is read through the caches and its 2400 bins live in global memory."""
    rows, W = 4, 24000
    x = _input(kind, rows, W, seed=24)
    truth = lpfilter_truth(x)
    first = None
    for what, got in _every_way(rec, x):
        if first is None:
            first = got
            _holds(got, x, "%d x %d %s, %s" % (rows, W, kind, what), truth)
        else:
            _same(got, first, what)
    # a row is filtered the same way whatever else is in the batch
    _same(rec.lowpass_rows(x[2]), first[2], "one row of the batch alone")


def test_one_column_and_batch_independence(rec):
    x = np.random.default_rng(5).uniform(0.0001, 1.0, (7, 1))
    _same(rec.lowpass_rows(x), x, "W = 1 blanks nothing")
    x = _input("sums", 1000, 640, seed=6)
    whole = rec.lowpass_rows(x)
    _same(rec.lowpass_rows(x[777]), whole[777], "a row alone and in a batch that fills the grid")
    _same(rec.lowpass_rows(x[990:]), whole[990:], "ten rows")


FLAGS = [(1, 0), (0, 0), (1, 1), (0, 1)]   # (donotnormalize, rowwisenormalize)


@pytest.mark.parametrize("dt", ["u16", "f32"])
@pytest.mark.parametrize("dnn,rwn", FLAGS)
def test_capture_with_lowpass_is_the_filter_on_the_capture(dnn, rwn, dt):
    W, H = GEOM["width"], GEOM["height"]
    kw = dict(rowwisenormalize=rwn, donotnormalize=dnn, movavgn=2)
    frames = _frames({"u16": np.uint16, "f32": np.float32}[dt], 5, H, W, seed=40 + dnn + 2 * rwn)
    a, b = Reconstructor(Config(**GEOM, **kw)), Reconstructor(Config(**GEOM, **kw))
    assert a.get_capture_options() == (False, False)
    a.set_capture_options(lowpass=True)
    assert a.get_capture_options() == (True, False)
    for i, role in enumerate((DARK, NONE, BACKGROUND)):
        device = i % 2 == 0
        fr = frames[i % 2:]
        if device:
            d = _DeviceFrames(fr, pad=3)
            got = a.capture_reference_device(role, d.ptr, d.dtype, d.n, d.pitch, out=True)
        else:
            got = a.capture_reference(role, fr, out=True)
        plain = b.capture_reference(role, fr, out=True)                     # the same capture with the option off ...
        model = capture_model.capture(role, fr, **kw)
        _same(plain, model, "role %d, option off" % role)
        _same(got, b.lowpass_rows(plain), "role %d: not the filter on the plain capture" % role)   # ... then the same kernel
        _holds(got, model, "capture role %d dnn %d rwn %d %s" % (role, dnn, rwn, dt))
        if role != NONE:
            _same(a.get_reference(role), got, "fdoct_get_reference, role %d" % role)
    # what the chain consumes: a handle given the filtered doubles through the setters is in the same state
    b.set_dark(a.get_reference(DARK))
    b.set_background(a.get_reference(BACKGROUND))
    assert a.export_state().tobytes() == b.export_state().tobytes()
    live = _frames(np.uint16, 2, H, W, seed=77)
    ba, da = a.process(live)
    bb, db = b.process(live)
    assert np.array_equal(ba.view(np.uint32), bb.view(np.uint32)) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    # PI is never filtered
    got = a.capture_reference(PI, frames[:1], out=True)
    _same(got, capture_model.capture(PI, frames[:1], **kw), "PI with the option on")
    # a clone carries the options
    c = a.clone_to_device(0) if hasattr(a, "clone_to_device") else None
    if c is not None:
        assert c.get_capture_options() == (True, False)
        c.close()
    a.close()
    b.close()


def test_sim_plain_copies_are_not_filtered():
    W, H = GEOM["width"], GEOM["height"]
    kw = dict(rowwisenormalize=1, donotnormalize=0, movavgn=3)
    rec = Reconstructor(Config(**GEOM, variant=VARIANT_SIM, **kw))
    frames = _frames(np.uint16, 3, H, W, seed=9)
    rec.set_capture_options(lowpass=True, raw_accumulate=True)
    for role in (BACKGROUND, PI):
        _same(rec.capture_reference(role, frames[:1], out=True), frames[0].astype(np.float64), "sim, role %d" % role)
    model = capture_model.capture(DARK, frames, sim=True, **kw)               # the sim variant's accumulating roles are filtered
    got = rec.capture_reference(DARK, frames, out=True)
    _holds(got, model, "sim, DARK")
    rec.close()


@pytest.mark.parametrize("dt", ["u16", "f32"])
def test_raw_accumulate_skips_the_moving_average(dt):
    W, H = GEOM["width"], GEOM["height"]
    frames = _frames({"u16": np.uint16, "f32": np.float32}[dt], 4, H, W, seed=12)
    for dnn, rwn in FLAGS:
        kw = dict(rowwisenormalize=rwn, donotnormalize=dnn)
        rec = Reconstructor(Config(**GEOM, movavgn=3, **kw))
        for role in (BACKGROUND, DARK, NONE, PI):
            fr = frames[:1] if role == PI else frames
            rec.set_capture_options(raw_accumulate=True)
            assert rec.get_capture_options() == (False, True)
            _same(rec.capture_reference(role, fr, out=True), capture_model.capture(role, fr, movavgn=0, **kw), "raw, role %d" % role)
            rec.set_capture_options()
            _same(rec.capture_reference(role, fr, out=True), capture_model.capture(role, fr, movavgn=3, **kw), "off, role %d" % role)
        rec.close()


def test_refusals_enqueue_nothing(rec):
    lib, h = rec.lib, rec.h
    x = np.random.default_rng(1).uniform(0.0, 1.0, (4, 64))
    out = np.full((4, 64), -7.0)
    H, D = capi.MEM_HOST, capi.MEM_DEVICE
    d = _DeviceRows(x)
    d_out = _DeviceRows(out)

    def refused(rc, text):
        assert rc == -1, rc
        assert text in lib.fdoct_last_error(h).decode(), lib.fdoct_last_error(h)
        rec.synchronize()
        assert np.all(out == -7.0)
        _same(d.host(), x)
        _same(d_out.host(), out)

    refused(lib.fdoct_lowpass_rows(h, None, H, 4, 64, 0, out.ctypes.data, H), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, H, 4, 64, 0, None, H), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, d.ptr, D, 4, 64, 0, None, D), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, H, 0, 64, 0, out.ctypes.data, H), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, H, -1, 64, 0, out.ctypes.data, H), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, H, 4, 0, 0, out.ctypes.data, H), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, 5, 4, 64, 0, out.ctypes.data, H), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, d.ptr, D, 4, 64, 0, d_out.ptr, 7), "bad arguments")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, H, 4, 64, 64 * 8 - 8, out.ctypes.data, H), "pitch smaller than a row")
    refused(lib.fdoct_lowpass_rows(h, d.ptr, D, 4, 64, 8, d_out.ptr, D), "pitch smaller than a row")
    refused(lib.fdoct_lowpass_rows(h, x.ctypes.data, H, 2, 64, 64 * 8 + 4, out.ctypes.data, H), "aligned")
    refused(lib.fdoct_lowpass_rows(h, d.ptr, D, 2, 64, 64 * 8 + 4, d_out.ptr, D), "aligned")
    refused(lib.fdoct_lowpass_rows(h, d.ptr + 4, D, 2, 64, 0, d_out.ptr, D), "aligned")
    refused(lib.fdoct_get_capture_options(h, None, None), "no output")
    assert rec.get_capture_options() == (False, False)


def test_host_harness_captures_a_filtered_background(tmp_path):
    """host/bscanfft_sim --capture-background 16 --capture-lowpass: the C++ caller's filtered background against the model."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    exe = os.path.join(ROOT, "host", "bscanfft_sim")
    W, H, N, D = 128, 96, 1024, 512
    frames = _frames(np.uint16, 18, H, W, seed=56)
    f_ocv = str(tmp_path / "frames.ocv")
    io.write_ocv(f_ocv, frames.reshape(18 * H, W))
    for flags, kw in ((["--capture-lowpass"], dict(movavgn=0)), (["--capture-lowpass", "--capture-raw"], dict(movavgn=0))):
        prefix = str(tmp_path / ("out%d" % len(flags)))
        cmd = [exe, "--frames", f_ocv, "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N),
               "--numdisplaypoints", str(D), "--out", prefix, "--capture-background", "16"] + flags
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
        got = np.fromfile(prefix + "_background.f64", np.float64).reshape(H, W)
        _holds(got, capture_model.capture(BACKGROUND, frames[:16], **kw), "bscanfft_sim " + " ".join(flags))
        bscan = np.fromfile(prefix + "_bscan.f32", np.float32).reshape(-1, D, H)
        assert bscan.shape[0] == 2
        # the Python path on the same frames: the same background to the bit, the same B-scans
        rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
        rec.set_capture_options(lowpass=True, raw_accumulate=len(flags) > 1)
        _same(rec.capture_reference(BACKGROUND, frames[:16], out=True), got)
        pb, _ = rec.process(frames[16:], layout=capi.LAYOUT_TRANSPOSED)
        rec.close()
        assert np.array_equal(bscan.view(np.uint32), pb.view(np.uint32))
