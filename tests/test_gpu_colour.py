"""GPU tests of the colour front end (include/fdoct_colour.h) against tests/colour_model.py and against the library's own mono
and FDOCT_F64 paths.  Every comparison is bit for bit (doubles as uint64 words): the select path is integer arithmetic, the sum
path is IEEE double operations in a stated order, and behind the stage a call is the call a mono handle makes."""
import os
import subprocess

import numpy as np
import pytest

import colour_model
from colour_model import bits
from fdoct_amd import (DTYPE_F64, DTYPE_U8, LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED, REF_BACKGROUND, REF_NONE, REF_PI, Config,
                       FdoctError, Reconstructor, capi, io, synth)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = [(1, 1), (2, 2), (4, 4), (3, 1), (1, 2)]
WEBCAM = dict(width=640, numfftpoints=640, numdisplaypoints=320)    # build/BscanFFTwebcam.ini: 640 points, M = 1
C1 = dict(width=1024, numfftpoints=1024, numdisplaypoints=512)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(bits(got), bits(want)), what


def _bgr(seed, n, h, w):
    """n seeded random frames, then an all-zero and an all-255 one."""
    f = np.random.default_rng(seed).integers(0, 256, (n + 2, h, w, 3), dtype=np.uint8)
    f[n] = 0
    f[n + 1] = 255
    return f


class _Device:
    """An array's bytes in device memory: rows of `row_bytes` at pitch row_bytes + pad, `offset` bytes past a 16-byte boundary."""

    def __init__(self, a, row_bytes=None, pad=0, offset=0):
        import torch
        raw = np.ascontiguousarray(a).view(np.uint8)
        row_bytes = raw.size if row_bytes is None else row_bytes
        rows = raw.reshape(-1, row_bytes)
        padded = np.zeros((rows.shape[0], row_bytes + pad), np.uint8)
        padded[:, :row_bytes] = rows
        buf = np.zeros(offset + padded.size, np.uint8)
        buf[offset:] = padded.ravel()
        self.t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + offset
        self.pitch = row_bytes + pad


def _device_out(shape, dtype):
    import torch
    t = torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # the fill runs on torch's stream, the library on the handle's: it must have landed first
    return t, lambda: t.cpu().numpy().view(dtype).reshape(shape)


def _rec(geom, height, averages=1, **kw):
    cfg = Config(height=height, averages=averages, device=0, **geom, **kw)
    rec = Reconstructor(cfg)
    rec.set_background(synth.make_background(cfg.width))
    return rec


@pytest.fixture(scope="module")
def rec():
    r = _rec(WEBCAM, 8)
    yield r
    r.close()


# ---- 1. the stage on its own against the model
def _width_for(bins, alt):
    """Raw widths the factors divide whose outputs are / are not whole groups of 16 (and an odd one for 1 x 1)."""
    return {(1, 1): (640, 637), (2, 2): (640, 1004), (4, 4): (640, 1000), (3, 1): (768, 639), (1, 2): (656, 637)}[bins][alt]


@pytest.mark.parametrize("bins", BINS)
def test_extract_equals_the_model_from_host_memory(rec, bins):
    for alt in (0, 1):
        w = _width_for(bins, alt)
        f = _bgr(31 + alt, 2, 24, w)
        for c in range(3):
            for mediann in colour_model.MEDIANS:
                _same(rec.colour_extract(f, c, mediann, *bins), colour_model.extract(f, c, mediann, *bins), "host c=%d median %d bins %s w=%d" % (c, mediann, bins, w))
        _same(rec.colour_extract(f, 3, 0, *bins), colour_model.extract(f, 3, 0, *bins), "host sum bins %s w=%d" % (bins, w))
    # a padded host view passes its pitch on
    wide = _bgr(5, 1, 24, 648)
    view = wide[:, :, :636 if bins[0] == 3 else 640]
    assert not view.flags.c_contiguous
    _same(rec.colour_extract(view, 1, 0, *bins), colour_model.extract(view, 1, 0, *bins), "padded host rows")


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("pad,offset", [(0, 0), (5, 0), (0, 1), (16, 0), (7, 1)])
def test_extract_equals_the_model_from_device_memory_at_any_pitch_and_base(rec, bins, pad, offset):
    import torch
    for alt in (0, 1):
        w = _width_for(bins, alt)
        f = _bgr(47 + alt, 1, 16, w)
        n, h = f.shape[0], f.shape[1]
        d = _Device(f, row_bytes=3 * w, pad=pad, offset=offset)
        for c, mediann in [(0, 0), (1, 0), (2, 0), (3, 0), (1, 3), (2, 5), (0, 7)]:
            want = colour_model.extract(f, c, mediann, *bins)
            out, read = _device_out(want.shape, want.dtype)
            rec.colour_extract_device(d.ptr, n, w, h, d.pitch, c, out.data_ptr(), mediann, *bins)
            rec.synchronize()
            _same(read(), want, "device c=%d median %d bins %s w=%d pad %d offset %d" % (c, mediann, bins, w, pad, offset))
    torch.cuda.synchronize()


def test_extract_writes_to_an_unaligned_device_output(rec):
    f = _bgr(3, 1, 8, 50)
    d = _Device(f)
    for c in (2, 3):
        want = colour_model.extract(f, c)
        out, _ = _device_out((want.nbytes + 8,), np.uint8)
        off = 8 if c == 3 else 1   # doubles stay aligned to themselves
        rec.colour_extract_device(d.ptr, 3, 50, 8, 0, c, out.data_ptr() + off)
        rec.synchronize()
        got = out.cpu().numpy()
        _same(got[off:off + want.nbytes].view(want.dtype).reshape(want.shape), want)
        assert not got[:off].any() and not got[off + want.nbytes:].any()


# ---- 2. / 3. behind the stage the call is a mono handle's
def _process_both_ways(rec, frames, dtype, layout):
    """(linear, dB) from process (host memory) and from process_device (device memory)."""
    hb, hd = rec.process(frames, layout=layout)
    a = np.ascontiguousarray(frames)
    d = _Device(a, row_bytes=a.strides[1])
    mag, rmag = _device_out(hb.shape, np.float32)
    db, rdb = _device_out(hb.shape, np.float32)
    rec.process_device(d.ptr, dtype, a.shape[0], d.pitch, mag.data_ptr(), db.data_ptr(), layout)
    rec.synchronize()
    return hb, hd, rmag(), rdb()


FRONT_ENDS = [(0, (1, 1)), (0, (2, 2)), (3, (2, 2)), (5, (1, 1)), (0, (4, 4)), (7, (3, 1))]


@pytest.mark.parametrize("geom", [WEBCAM, C1], ids=["webcam", "C1"])
@pytest.mark.parametrize("averages", [1, 2])
@pytest.mark.parametrize("mediann,bins", FRONT_ENDS)
def test_select_equals_the_mono_handle_on_that_channel(geom, averages, mediann, bins):
    H = 12
    f = _bgr(71, 2, H * bins[1], geom["width"] * bins[0])
    colour, mono = _rec(geom, H, averages), _rec(geom, H, averages)
    try:
        for r in (colour, mono):
            r.set_frontend(mediann, *bins)
        for c in range(3):
            colour.set_colour_input(c)
            assert colour.get_colour_input() == c and mono.get_colour_input() == -1
            for layout in (LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED):
                got = _process_both_ways(colour, f, DTYPE_U8, layout)
                want = _process_both_ways(mono, np.ascontiguousarray(f[..., c]), DTYPE_U8, layout)
                for g, w, what in zip(got, want, ("process linear", "process dB", "process_async linear", "process_async dB")):
                    _same(g, w, "%s c=%d layout %d" % (what, c, layout))
                assert np.isfinite(got[0]).all() and got[0].any()
    finally:
        colour.close()
        mono.close()


def test_select_on_the_shapes_whose_kernel_bins_in_its_own_loads():
    """8-bit rows of at most 320 samples with 2 x 2 binning: the mono handle's run-time compiled kernel bins by itself."""
    geom = dict(width=320, numfftpoints=1024, numdisplaypoints=256)
    f = _bgr(13, 2, 16, 640)
    colour, mono = _rec(geom, 8), _rec(geom, 8)
    try:
        for r in (colour, mono):
            r.set_frontend(0, 2, 2)
        colour.set_colour_input(1)
        got = _process_both_ways(colour, f, DTYPE_U8, LAYOUT_ROWMAJOR)
        want = _process_both_ways(mono, np.ascontiguousarray(f[..., 1]), DTYPE_U8, LAYOUT_ROWMAJOR)
        for g, w in zip(got, want):
            _same(g, w)
        assert colour.last_kernel() == mono.last_kernel()
    finally:
        colour.close()
        mono.close()


@pytest.mark.parametrize("geom", [WEBCAM, C1], ids=["webcam", "C1"])
@pytest.mark.parametrize("averages,movavgn", [(1, 0), (2, 0), (1, 2)])
@pytest.mark.parametrize("bins", BINS)
def test_sum_equals_the_f64_path_on_the_models_frames(geom, averages, movavgn, bins):
    H = 12
    f = _bgr(91, 2, H * bins[1], geom["width"] * bins[0])
    colour, mono = _rec(geom, H, averages, movavgn=movavgn), _rec(geom, H, averages, movavgn=movavgn)
    try:
        colour.set_frontend(0, *bins)
        colour.set_colour_input(3)
        doubles = colour_model.extract(f, 3, 0, *bins)
        for layout in (LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED):
            got = _process_both_ways(colour, f, DTYPE_U8, layout)
            want = _process_both_ways(mono, doubles, DTYPE_F64, layout)
            for g, w, what in zip(got, want, ("process linear", "process dB", "process_async linear", "process_async dB")):
                _same(g, w, "%s layout %d" % (what, layout))
            assert np.isfinite(got[0]).all() and got[0].any()
    finally:
        colour.close()
        mono.close()


# ---- 4. the other entry points
@pytest.mark.parametrize("c,mediann,bins", [(0, 0, (1, 1)), (1, 3, (2, 2)), (2, 0, (4, 4)), (3, 0, (1, 1)), (3, 0, (2, 2)), (3, 0, (3, 1))])
@pytest.mark.parametrize("lowpass", [False, True])
def test_capture_and_minmax_equal_the_calls_on_the_models_frames(c, mediann, bins, lowpass):
    H, geom = 10, WEBCAM
    f = _bgr(17, 4, H * bins[1], geom["width"] * bins[0])[:4]
    model = colour_model.extract(f, c, mediann, *bins)
    colour, mono = _rec(geom, H), _rec(geom, H)
    try:
        colour.set_frontend(mediann, *bins)
        colour.set_colour_input(c)
        for r in (colour, mono):
            r.set_capture_options(lowpass=lowpass)
        d = _Device(f, row_bytes=f.strides[1], pad=3, offset=1)
        dm = _Device(model, row_bytes=model.strides[1])
        mdt = DTYPE_F64 if c == 3 else DTYPE_U8
        # background over averagestoggle = 4 frames, from host and from device memory
        _same(colour.capture_reference(REF_BACKGROUND, f, out=True), mono.capture_reference(REF_BACKGROUND, model, out=True), "background, host")
        _same(colour.get_reference(REF_BACKGROUND), mono.get_reference(REF_BACKGROUND))
        _same(colour.capture_reference_device(REF_BACKGROUND, d.ptr, DTYPE_U8, 4, d.pitch, out=True),
              mono.capture_reference_device(REF_BACKGROUND, dm.ptr, mdt, 4, dm.pitch, out=True), "background, device")
        # the p key: one frame
        _same(colour.capture_reference(REF_PI, f[:1], out=True), mono.capture_reference(REF_PI, model[:1], out=True), "pi")
        _same(colour.get_reference(REF_PI), mono.get_reference(REF_PI))
        # no role: the result only
        before = colour.get_reference(REF_BACKGROUND)
        _same(colour.capture_reference(REF_NONE, f[1:3], out=True), mono.capture_reference(REF_NONE, model[1:3], out=True), "none")
        _same(colour.get_reference(REF_BACKGROUND), before)
        # "Max intensity"
        for got, want in zip(colour.frame_minmax(f), mono.frame_minmax(model)):
            _same(got, want, "frame_minmax, host")
        lo, rlo = _device_out((4,), np.float64)
        hi, rhi = _device_out((4,), np.float64)
        colour.frame_minmax_device(d.ptr, DTYPE_U8, 4, d.pitch, lo.data_ptr(), hi.data_ptr())
        colour.synchronize()
        _same(rlo(), model.reshape(4, -1).min(axis=1).astype(np.float64))
        _same(rhi(), model.reshape(4, -1).max(axis=1).astype(np.float64))
    finally:
        colour.close()
        mono.close()


def test_a_refused_call_changes_nothing_and_the_next_valid_call_succeeds():
    H, geom = 8, WEBCAM
    f = _bgr(23, 2, H, geom["width"])
    r = _rec(geom, H)
    try:
        r.set_colour_input(3)
        good_b, good_d = r.process(f)
        r.capture_reference(REF_BACKGROUND, f[:2])
        kept = r.get_reference(REF_BACKGROUND)
        r.set_frontend(3, 1, 1)            # the sum with a median: every frame-taking call refuses
        d = _Device(f, row_bytes=f.strides[1])
        out, _ = _device_out(good_b.shape, np.float32)
        calls = [lambda: r.process(f), lambda: r.process_device(d.ptr, DTYPE_U8, 4, d.pitch, out.data_ptr(), None),
                 lambda: r.capture_reference(REF_BACKGROUND, f[:2]), lambda: r.capture_reference_device(REF_PI, d.ptr, DTYPE_U8, 1, d.pitch),
                 lambda: r.frame_minmax(f)]
        for call in calls:
            with pytest.raises(FdoctError) as e:
                call()
            assert e.value.code == -2 and "medianBlur" in str(e.value)
            assert r.get_colour_input() == 3
            _same(r.get_reference(REF_BACKGROUND), kept)
        assert not out.cpu().numpy().any()
        # a wrong sample type is refused likewise, with the reason
        r.set_frontend(0, 1, 1)
        with pytest.raises(FdoctError) as e:
            r.process(np.zeros((1, H, geom["width"]), np.uint16))
        assert e.value.code == -2 and "8-bit" in str(e.value)
        with pytest.raises(FdoctError) as e:
            r.frame_minmax(np.zeros((1, H, geom["width"]), np.float64))
        assert e.value.code == -2
        with pytest.raises(FdoctError) as e:
            r.set_colour_input(4)
        assert e.value.code == -1 and r.get_colour_input() == 3
        with pytest.raises(FdoctError):
            r.set_colour_input(-2)
        # sizes the bin factors do not divide, the stage on its own
        with pytest.raises(FdoctError) as e:
            r.colour_extract(f[:, :, :639], 0, 0, 2, 1)
        assert e.value.code == -1
        # ... and the handle works as before
        r.set_background(synth.make_background(geom["width"]))
        b, dbv = r.process(f)
        _same(b, good_b)
        _same(dbv, good_d)
        # switched off, the handle takes mono frames again, bit for bit as a handle that never had the setting
        r.set_colour_input(-1)
        mono = _rec(geom, H)
        try:
            m = np.ascontiguousarray(f[..., 0])
            for g, w in zip(r.process(m), mono.process(m)):
                _same(g, w)
        finally:
            mono.close()
    finally:
        r.close()


# ---- 5. the host pipeline
@pytest.mark.parametrize("c", [1, 3])
def test_a_chunked_host_batch_equals_the_unchunked_device_call(c):
    """80 colour frames of 640 x 480 (74 MB): fdoct_process cuts pageable batches into four or more 16 MB chunks and pinned
    ones into 8 MB chunks; the chunk sizes, strides and staging all come from the 3-byte pixel rows."""
    n, H, W = 80, 480, 640
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    r = _rec(WEBCAM, H)
    pinned = []
    try:
        r.set_colour_input(c)
        d = _Device(f, row_bytes=3 * W)
        shape = (n, H, WEBCAM["numdisplaypoints"])
        mag, rmag = _device_out(shape, np.float32)
        db, rdb = _device_out(shape, np.float32)
        r.process_device(d.ptr, DTYPE_U8, n, d.pitch, mag.data_ptr(), db.data_ptr())
        r.synchronize()
        want_b, want_d = rmag(), rdb()
        assert np.isfinite(want_b).all() and want_b.any()
        got_b, got_d = r.process(f)                                  # pageable memory
        _same(got_b, want_b, "pageable, linear")
        _same(got_d, want_d, "pageable, dB")
        pin_f, pin_b, pin_d = capi.PinnedArray(f.shape, np.uint8), capi.PinnedArray(shape, np.float32), capi.PinnedArray(shape, np.float32)
        pinned = [pin_f, pin_b, pin_d]
        pin_f.array[...] = f
        pin_b.array[...] = 0
        pin_d.array[...] = 0
        r.process(pin_f.array, out_bscan=pin_b.array, out_db=pin_d.array)   # fdoct_host_alloc memory
        _same(pin_b.array, want_b, "pinned, linear")
        _same(pin_d.array, want_d, "pinned, dB")
    finally:
        r.close()
        for p in pinned:
            p.free()


# ---- 6. clone and export
def test_the_clone_carries_the_setting_and_the_state_blob_does_not():
    H = 8
    f = _bgr(29, 1, H, WEBCAM["width"])
    r = _rec(WEBCAM, H)
    try:
        r.set_colour_input(2)
        clone = r.clone_to_device(0)
        try:
            assert clone.get_colour_input() == 2
            for g, w in zip(clone.process(f), r.process(f)):
                _same(g, w)
        finally:
            clone.close()
        blob = r.export_state()
        fresh = Reconstructor(r.cfg)
        other = Reconstructor(r.cfg)
        try:
            fresh.import_state(blob)
            assert fresh.get_colour_input() == -1
            other.set_colour_input(1)
            other.import_state(blob)
            assert other.get_colour_input() == 1
            for g, w in zip(fresh.process(np.ascontiguousarray(f[..., 2])), r.process(f)):
                _same(g, w)
        finally:
            fresh.close()
            other.close()
    finally:
        r.close()


# ---- 7. the C++ caller
@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    exe = os.path.join(ROOT, "host", "bscanfft_sim")
    assert os.path.exists(exe)
    return exe


@pytest.mark.parametrize("channel", [1, 3])
def test_bscanfft_sim_channel_gives_the_python_calls_bscan(harness, tmp_path, channel):
    W, H, N, D = 128, 96, 1024, 512
    f = _bgr(37, 5, H, W)[:6]
    frames_file = str(tmp_path / "webcam.ocv")
    io.write_ocv(frames_file, f.reshape(6 * H, W, 3))
    prefix = str(tmp_path / "out")
    cmd = [harness, "--frames", frames_file, "--capture-background", "2", "--max-intensity", "--channel", str(channel), "--width", str(W),
           "--height", str(H), "--bits", "8", "--numfftpoints", str(N), "--numdisplaypoints", str(D), "--out", prefix]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
    r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, device=0))
    try:
        r.set_colour_input(channel)
        r.capture_reference(REF_BACKGROUND, f[:2])
        bscan, db = r.process(f[2:], layout=LAYOUT_TRANSPOSED)
        _, hi = r.frame_minmax(f[2:])
        gray = r.display(db[0])
    finally:
        r.close()
    ocv = io.read_ocv(prefix + "_bscan001.ocv")
    _same(ocv, bscan[0], "_bscan001.ocv")
    _same(np.fromfile(prefix + "_bscan.f32", np.float32).reshape(-1, D, H), bscan)
    _same(np.fromfile(prefix + "_bscandb.f32", np.float32).reshape(-1, D, H), db)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Max intensity")]
    assert lines == ["Max intensity = %d" % int(np.floor(v)) for v in hi]
    pgm = open(prefix + "_bscan001.pgm", "rb").read()
    assert pgm.endswith(gray.tobytes())
    # a mono dump is refused with --channel, and a colour one without it
    mono_file = str(tmp_path / "mono.ocv")
    io.write_ocv(mono_file, f[..., 0].reshape(6 * H, W))
    bad = subprocess.run([a if a != frames_file else mono_file for a in cmd], capture_output=True, text=True, timeout=240)
    assert bad.returncode != 0 and "3-channel" in bad.stderr
