"""GPU test of the staging buffers the side entry points share (fdoct_amd/csrc/fdoct_stage.h, stage_reserve / stage_upload / stage_finish in fdoct_ctx.h): ONE handle
takes host-memory calls of every such entry point, a large shape, then a small one, then the large one again, so that a stale
pointer or a wrong offset in the two shared buffers shows.  Every result equals, byte for byte, the same call made once on a
fresh handle with device-memory arguments (torch tensors through the *_device wrappers) -- fdoct_frontend, which has no device
form, a fresh handle's host call.  A process call at the end shows the chain's own workspaces undisturbed.  No tolerance."""
import numpy as np
import pytest

from fdoct_amd import Config, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
W, H, N, D = 64, 8, 64, 32


def _rec():
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(synth.make_background(W))
    return rec


def _same(got, want, what):
    got, want = (got, want) if isinstance(got, (tuple, list)) else ((got,), (want,))
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, "%s, output %d: one side is missing" % (what, k)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s, output %d: %s %s against %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), "%s, output %d: %d elements differ" % (what, k, int((g != w).sum()))


class _Device:
    """One call on a fresh handle with device-memory arguments."""

    def __init__(self):
        import torch
        self.torch = torch
        self.rec = _rec()

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def empty(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device="cuda")

    def run(self, fn, *outs):
        self.torch.cuda.synchronize()
        res = fn(self.rec)
        self.rec.synchronize()
        got = tuple(None if o is None else o.cpu().numpy() for o in outs)
        self.rec.close()
        return got if outs else res


def _db(n, depths, layout, seed):
    a = np.random.default_rng(seed).uniform(-60.0, 10.0, (n, depths, H)).astype(np.float32)  # (n, depths, ascans): the D x H pictures
    return np.ascontiguousarray(a if layout == TR else np.transpose(a, (0, 2, 1)))


# ---- each entry point: on(rec) is the host-memory call, dev() the device-memory call on a fresh handle ---------------------
def _ascan_minmax(n, depths, layout):
    a = _db(n, depths, layout, 1)

    def dev():
        d = _Device()
        t, lo, hi = d.up(a), d.empty(n, d.torch.float32), d.empty(n, d.torch.float32)
        return d.run(lambda r: r.ascan_minmax_device(t.data_ptr(), n, depths, H, 3, lo.data_ptr(), hi.data_ptr(), layout), lo, hi)
    return lambda rec: rec.ascan_minmax(a, 3, layout), dev


def _roi_mean(n, depths, layout):
    a = _db(n, depths, layout, 2)

    def dev():
        d = _Device()
        t, out = d.up(a), d.empty(n, d.torch.float64)
        return d.run(lambda r: r.roi_mean_device(t.data_ptr(), n, depths, H, 2, 1, 3, out.data_ptr(), layout), out)
    return lambda rec: (rec.roi_mean(a, 2, 1, 3, layout),), dev


def _peakhold(n, depths, layout):
    a = _db(n, depths, layout, 3)

    def on(rec):
        rec.set_peakhold_roi(1, 1, 4, 3, 2)  # (resets the column holds; the scalar one is cleared by hand)
        rec.clear_peakhold(2)
        rec.peakhold(2, a, layout)
        return rec.peakhold_values(2)

    def dev():  # (the values are read before the handle closes)
        d = _Device()
        t = d.up(a)
        d.rec.set_peakhold_roi(1, 1, 4, 3, 2)
        d.torch.cuda.synchronize()
        d.rec.peakhold_device(2, t.data_ptr(), n, depths, H, layout)
        res = d.rec.peakhold_values(2)
        d.rec.close()
        return res
    return on, dev


def _frames(n):
    return np.random.default_rng(10 + n).integers(0, 4096, (n, H, W)).astype(np.uint16)


def _frame_minmax(n):
    f = _frames(n)

    def dev():
        d = _Device()
        t, lo, hi = d.up(f), d.empty(n, d.torch.float64), d.empty(n, d.torch.float64)
        return d.run(lambda r: r.frame_minmax_device(t.data_ptr(), capi.DTYPE_U16, n, 0, lo.data_ptr(), hi.data_ptr()), lo, hi)
    return lambda rec: rec.frame_minmax(f), dev


def _capture_dark(n):
    f = _frames(n)

    def dev():
        d = _Device()
        t = d.up(f)
        return (d.run(lambda r: r.capture_reference_device(capi.REF_DARK, t.data_ptr(), capi.DTYPE_U16, n, 0, out=True)),)
    return lambda rec: (rec.capture_reference(capi.REF_DARK, f, out=True),), dev


def _lowpass(rows, width):
    pad = np.random.default_rng(20 + rows).uniform(-1.0, 1.0, (rows, width + 3))  # a pitch of width + 3 doubles

    def on(rec):
        out = np.zeros_like(pad)
        rec.lowpass_rows(pad[:, :width], out=out[:, :width])
        return (np.ascontiguousarray(out[:, :width]),)

    def dev():
        d = _Device()
        t, out = d.up(pad), d.empty((rows, width + 3), d.torch.float64)
        got, = d.run(lambda r: r.lowpass_rows_device(t.data_ptr(), rows, width, 8 * (width + 3), out.data_ptr()), out)
        return (np.ascontiguousarray(got[:, :width]),)
    return on, dev


def _bscan_bin(with_jscan, want):
    a = np.random.default_rng(30).uniform(0.0, 50.0, (2, H, D)).astype(np.float32)  # row-major: (n, ascans, depths)
    j = np.random.default_rng(31).uniform(0.0, 20.0, (H, D)).astype(np.float32) if with_jscan else None

    def dev():
        d = _Device()
        t, tj = d.up(a), None if j is None else d.up(j)
        outs = [d.empty((2, H, D), d.torch.float32) if w else None for w in want]
        return d.run(lambda r: r.bscan_bin_device(t.data_ptr(), 2, D, H, 2, 2, *[None if o is None else o.data_ptr() for o in outs],
                                                  d_jscan_ptr=None if tj is None else tj.data_ptr()), *outs)
    return lambda rec: rec.bscan_bin(a, 2, 2, jscan=j, want_bscan=want[0], want_db=want[1]), dev


def _display(colour):
    a = np.random.default_rng(40).uniform(-70.0, 5.0, (2, 6, 7)).astype(np.float32)

    def on(rec):
        res = rec.display(a, clampupper=True, colour=colour)
        return res if colour else (res, None)

    def dev():
        d = _Device()
        t, gray = d.up(a), d.empty((2, 6, 7), d.torch.uint8)
        bgr = d.empty((2, 6, 7, 3), d.torch.uint8) if colour else None
        return d.run(lambda r: r.display_device(t.data_ptr(), 2, 6, 7, gray.data_ptr(), bgr.data_ptr() if colour else None,
                                                clampupper=True), gray, bgr)
    return on, dev


def _lockin():
    b = np.random.default_rng(50).uniform(0.0, 50.0, (2, H, D)).astype(np.float32)
    j = np.random.default_rng(51).uniform(0.0, 50.0, (H, D)).astype(np.float32)

    def dev():
        d = _Device()
        tb, tj, out = d.up(b), d.up(j), d.empty((2, H, D), d.torch.float32)
        return d.run(lambda r: r._check(r.lib.fdoct_lockin_db(r.h, tb.data_ptr(), tj.data_ptr(), capi.MEM_DEVICE, 2, j.size, out.data_ptr())),
                     out)
    return lambda rec: (rec.lockin_db(b, j),), dev


def _frontend():
    raw = np.random.default_rng(60).integers(0, 4096, (1, 16, 128)).astype(np.uint16)

    def fresh():
        rec = _rec()
        res = rec.frontend(raw, 3, 2, 2)
        rec.close()
        return (res,)
    return lambda rec: (rec.frontend(raw, 3, 2, 2),), fresh


def _colour(channelnum):
    bgr = np.random.default_rng(70).integers(0, 256, (2, H, W, 3)).astype(np.uint8)

    def dev():
        d = _Device()
        t, out = d.up(bgr), d.empty((2, H, W), d.torch.float64 if channelnum == 3 else d.torch.uint8)
        return d.run(lambda r: r.colour_extract_device(t.data_ptr(), 2, W, H, 3 * W, channelnum, out.data_ptr()), out)
    return lambda rec: (rec.colour_extract(bgr, channelnum),), dev


def test_host_memory_calls_share_the_staging_buffers_and_match_device_memory_calls():
    large = [("ascan_minmax 3 x (8 x 32) %s" % ("D x H" if lay == TR else "H x D"), _ascan_minmax(3, D, lay)) for lay in (ROW, TR)]
    large += [("roi_mean 3 x (8 x 32) layout %d" % lay, _roi_mean(3, D, lay)) for lay in (ROW, TR)]
    large += [("peakhold 3 x (8 x 32) layout %d" % lay, _peakhold(3, D, lay)) for lay in (ROW, TR)]
    large += [("frame_minmax 5 frames", _frame_minmax(5)), ("capture_reference(DARK) 5 frames", _capture_dark(5)),
              ("lowpass_rows 8 x 64", _lowpass(8, 64)), ("bscan_bin with jscan, both outputs", _bscan_bin(True, (True, True))),
              ("display 6 x 7, gray and colour", _display(True)), ("lockin_db", _lockin()), ("frontend 16 x 128", _frontend()),
              ("colour_extract channel 1", _colour(1))]
    small = [("ascan_minmax 1 x (8 x 5) layout %d" % lay, _ascan_minmax(1, 5, lay)) for lay in (ROW, TR)]
    small += [("roi_mean 1 x (8 x 5) layout %d" % lay, _roi_mean(1, 5, lay)) for lay in (ROW, TR)]
    small += [("peakhold 1 x (8 x 5) layout %d" % lay, _peakhold(1, 5, lay)) for lay in (ROW, TR)]
    small += [("frame_minmax 2 frames", _frame_minmax(2)), ("capture_reference(DARK) 2 frames", _capture_dark(2)),
              ("lowpass_rows 3 x 20", _lowpass(3, 20)), ("bscan_bin, dB alone", _bscan_bin(False, (False, True))),
              ("bscan_bin, linear alone", _bscan_bin(True, (True, False))), ("display 6 x 7, gray only", _display(False)),
              ("colour_extract sum", _colour(3))]
    want = {what: dev() for what, (_, dev) in large + small}

    rec = _rec()
    calls = 0
    for rnd, cases in enumerate((large, small, large)):
        for what, (on, _) in cases:
            _same(on(rec), want[what], "round %d, %s" % (rnd, what))
            calls += 1
    print("%d host-memory calls on one handle equal %d device-memory calls on fresh handles, byte for byte" % (calls, len(want)))

    # the chain after all that: the handle's dark frame is the last capture's (5 frames), and so is the fresh handle's
    frames = synth.make_frames(0, 4, W, H)
    got = rec.process(frames)
    rec.close()
    fresh = _rec()
    fresh.capture_reference(capi.REF_DARK, _frames(5))
    _same(got, fresh.process(frames), "process after the side calls")
    fresh.close()


def test_process_single_shot_stages_through_the_plan_and_refuses_before_it_copies():
    """fdoct_process below the pipeline's threshold stages its host-memory arguments through the same plan (fdoct_stage.h) as the
    side entry points.  512 x 16 u16 frames, 512 points, 256 depths, 2 averages, 4 frames, called through the C ABI for what
    Reconstructor.process cannot reach: host frames at a padded pitch (1024 + 16 bytes) into device outputs, device frames into
    host outputs, host into host with one output wanted -- each, in both layouts, equal bit for bit to process() on the packed
    host arrays.  Then calls refused before anything is enqueued -- 3 frames with 2 averages, a handle without a background --
    with the code and text they have always had, after which the next good call still matches."""
    import torch
    w, hh, n, d = 512, 16, 512, 256
    cfg = Config(width=w, height=hh, numfftpoints=n, numdisplaypoints=d, averages=2)
    frames = synth.make_frames(11, 4, w, hh)
    padded = np.zeros((4, hh, w + 8), np.uint16)
    padded[:, :, :w] = frames
    rec = Reconstructor(cfg)
    rec.set_background(synth.make_background(w))
    U16, HOST, DEV = capi.DTYPE_U16, capi.MEM_HOST, capi.MEM_DEVICE

    def call(r, fr, space, nframes, pitch, mag, db, out_space, lay):
        ptr = lambda a: None if a is None else a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data
        return r.lib.fdoct_process(r.h, ptr(fr), U16, space, nframes, pitch, ptr(mag), ptr(db), out_space, lay)

    def refused(r, rc, code, text):
        assert rc == code and r.lib.fdoct_last_error(r.h).decode() == text, (rc, r.lib.fdoct_last_error(r.h))

    for lay in (ROW, TR):
        want_b, want_d = rec.process(frames, layout=lay)
        # host frames at a padded pitch into device outputs
        t_b, t_d = (torch.zeros(want_b.shape, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        assert call(rec, padded, HOST, 4, 2 * w + 16, t_b, t_d, DEV, lay) == 0
        _same((t_b.cpu().numpy(), t_d.cpu().numpy()), (want_b, want_d), "padded host frames into device outputs, layout %d" % lay)
        # device frames into host outputs
        t_f = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        got_b, got_d = np.zeros_like(want_b), np.zeros_like(want_d)
        assert call(rec, t_f, DEV, 4, 0, got_b, got_d, HOST, lay) == 0
        _same((got_b, got_d), (want_b, want_d), "device frames into host outputs, layout %d" % lay)
        # host into host, one output wanted
        got_d = np.zeros_like(want_d)
        assert call(rec, frames, HOST, 4, 0, None, got_d, HOST, lay) == 0
        _same(got_d, want_d, "host into host, dB only, layout %d" % lay)
        got_b = np.zeros_like(want_b)
        assert call(rec, padded, HOST, 4, 2 * w + 16, got_b, None, HOST, lay) == 0
        _same(got_b, want_b, "padded host into host, linear only, layout %d" % lay)
    # refused calls leave nothing behind
    want_b, want_d = rec.process(frames)
    got_b, got_d = np.zeros_like(want_b), np.zeros_like(want_d)
    refused(rec, call(rec, frames, HOST, 3, 0, got_b, got_d, HOST, ROW), -1, "nframes must be a multiple of averages")
    refused(rec, call(rec, frames, HOST, 4, 0, None, None, HOST, ROW), -1, "no output requested")
    refused(rec, call(rec, frames, HOST, 4, 2 * w - 2, got_b, got_d, HOST, ROW), -1, "pitch smaller than a row")
    assert not got_b.any() and not got_d.any()
    assert call(rec, frames, HOST, 4, 0, got_b, got_d, HOST, ROW) == 0
    _same((got_b, got_d), (want_b, want_d), "the good call after the refused ones")
    rec.close()
    bare = Reconstructor(cfg)
    got_b, got_d = np.zeros_like(want_b), np.zeros_like(want_d)
    refused(bare, call(bare, frames, HOST, 4, 0, got_b, got_d, HOST, ROW), -5, "no background set (fdoct_set_background)")
    assert not got_b.any()
    bare.set_background(synth.make_background(w))
    assert call(bare, frames, HOST, 4, 0, got_b, got_d, HOST, ROW) == 0
    _same((got_b, got_d), (want_b, want_d), "the good call after the one without a background")
    bare.close()
