"""GPU tests of fdoct_process_doppler (include/fdoct_doppler.h) behind every form of the chain, where tests/test_gpu_doppler.py runs
u16 host frames on two plain handles that have already made a complex call.  The rule throughout: process_doppler(frames, ...)
holds the bits of doppler(process_complex(frames), ...) on the same handle; the kernel family is asserted as
tests/test_gpu_complex_options.py asserts it; outputs start NaN-poisoned and come back finite.  The setups are
tests/complex_cases.py's.

  a. the first GPU call of a fresh handle is process_doppler -- the dry enqueue_complex, the upload, the real one, with ws_cx and
     ws_dop_bulk reserved in between and the run-time compile inside -- and a second call with twice the frames grows them;
  b. every chain option that puts a pass in front of the kernel or selects another one, on both forms, each kind on both axes
     and with and without the bulk correction;
  c. process_doppler_device: u8 / u16 / f32 frames in device memory with and without a row pitch, outputs at odd offsets between
     guard words, one output alone, a misaligned out_corr refused with nothing written;
  d. depths 1 / 63 / 64 / 65, both forms;
  e. state: a staged handle and one without a background refuse; refusals leave poisoned outputs alone; a clone gives its
     parent's bits."""
import numpy as np
import pytest

import complex_cases as cc
import doppler_edge_cases as de
import doppler_model as dm
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth
from test_gpu_complex_options import _complex, _handle, _ran
from test_gpu_doppler import NAMES, _bits, _poisoned, _raw, _untouched

pytestmark = pytest.mark.gpu


def _kw(axis, bulk, win=(3, 5), scale=2.0, min_power=0.0):
    return dict(axis=axis, lag=1, win=win, bulk=bulk, scale=scale, min_power=min_power)


def _params(kw):
    return capi.doppler_params(kw["axis"], kw["lag"], kw["win"], kw["bulk"], kw["scale"], kw["min_power"])


def _pd_raw(rec, frames, kw, want=NAMES, nframes=None, pitch=None, dtype=None):
    """fdoct_process_doppler itself on host frames with poisoned outputs: (return code, dict of the outputs)."""
    a = np.ascontiguousarray(frames)
    n = a.shape[0]
    shape = dm.pair_shape(kw["axis"], kw["lag"], max(n, kw["lag"] + 1), rec.cfg.height) + (rec.cfg.numdisplaypoints,)
    outs = {w: _poisoned(shape, w) for w in want}
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rc = rec.lib.fdoct_process_doppler(rec.h, a.ctypes.data, capi._NP2DT[a.dtype] if dtype is None else dtype, capi.MEM_HOST,
                                       n if nframes is None else nframes, a.strides[1] if pitch is None else pitch, _params(kw),
                                       ptr("phase"), ptr("corr"), ptr("power"), capi.MEM_HOST)
    return rc, outs


def _pd(rec, frames, kw, want=NAMES):
    rc, outs = _pd_raw(rec, frames, kw, want)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    return outs


def _composed(rec, frames, kw):
    """doppler() of what process_complex returns, both on `rec`: (the outputs, the complex A-scans)."""
    X = _complex(rec, frames)
    rc, outs = _raw(rec, X, **kw)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    return outs, X


def _same(got, want, what, live=True):
    """got holds want's bits and no poison; live: the phase is not 0 everywhere (a call that left zeros would pass the rest)."""
    assert set(got) <= set(want)
    for w, a in got.items():
        assert np.isfinite(a.view(np.float32)).all(), "%s: %s is not finite (an output bin was not written)" % (what, w)
        np.testing.assert_array_equal(_bits(a), _bits(want[w]), err_msg="%s: %s" % (what, w))
    if live and "phase" in got:
        assert np.count_nonzero(got["phase"]) > 0, what + ": every phase is 0"


def _median_power(X):
    return float(np.float32(np.median(np.abs(X) ** 2)))


# ---- a. the first call of a fresh handle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape", [("wave", cc.WAVE_SHAPE), ("generic", cc.GENERIC_SHAPE)], ids=["wave", "generic"])
def test_the_first_gpu_call_of_a_handle_is_process_doppler(route, shape):
    W, M, N, D = shape
    cfg = Config(width=W, height=cc.H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    frames = synth.make_frames(cc.FIRST_FRAME, 2 * cc.NF, W, cc.H)
    what = "first call, " + cc.shape_name(*shape)
    kw = _kw(dm.ASCANS, True)
    rec = _handle(cfg, synth.make_background(W).astype(np.float64))
    try:
        first = _pd(rec, frames[:cc.NF], kw)             # no workspace, table or run-time compiled kernel exists yet
        _ran(rec, route, what)
        want, _ = _composed(rec, frames[:cc.NF], kw)
        _same(first, want, what)
        more = _pd(rec, frames, kw)                      # twice the frames: ws_cx and ws_dop_bulk grow
        _ran(rec, route, what + ", twice the frames")
        want, _ = _composed(rec, frames, kw)
        _same(more, want, what + ", twice the frames")
        for w in NAMES:                                  # (and the first half of it is the first call's: A-scans pair within a frame)
            np.testing.assert_array_equal(_bits(more[w][:cc.NF]), _bits(first[w]), err_msg=w)
        again = _pd(rec, frames[:cc.NF], _kw(dm.FRAMES, True))
        want, _ = _composed(rec, frames[:cc.NF], _kw(dm.FRAMES, True))
        _same(again, want, what + ", frames axis afterwards")
    finally:
        rec.close()


# ---- b. every option -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.OPTION_CASES, ids=[c.name for c in cc.OPTION_CASES])
def test_every_option_on_both_forms(case):
    s = cc.option_setup(case)
    rec = _handle(s.cfg, s.yb, **s.hkw)
    try:
        for axis, bulk in de.option_axes(case):
            what = "%s, axis %d%s" % (case.name, axis, ", bulk" if bulk else "")
            X = _complex(rec, s.frames)
            _ran(rec, case.family, what)
            kw = _kw(axis, bulk, min_power=_median_power(X) if bulk else 0.0)
            rc, want = _raw(rec, X, **kw)
            assert rc == 0, rec.lib.fdoct_last_error(rec.h)
            got = _pd(rec, s.frames, kw)
            _ran(rec, case.family, what)
            _same(got, want, what)
            if bulk:    # the mask took some bins and left some
                zeros = np.count_nonzero(got["phase"] == 0)
                assert 0 < zeros < got["phase"].size, what
    finally:
        rec.close()


# ---- c. device memory ----------------------------------------------------------------------------------------------------------------
def _device_frames(frames, pad):
    """(device tensor, dtype code, nframes, row pitch in bytes): the frames in device memory, rows `pad` samples of junk apart."""
    import torch
    a = np.ascontiguousarray(frames)
    n, rows, w = a.shape
    row, step = w * a.itemsize, (w + pad) * a.itemsize
    host = np.full((n * rows, step), 0xA5, np.uint8)
    host[:, :row] = a.view(np.uint8).reshape(n * rows, row)
    return torch.from_numpy(host.reshape(-1)).cuda(), capi._NP2DT[a.dtype], n, step


def _device_complex(rec, dev, pitch):
    """process_complex_device on the same device frames: the complex A-scans the composition starts from."""
    import torch
    d_in, code, n, _ = dev
    H, D = rec.cfg.height, rec.cfg.numdisplaypoints
    d_out = torch.full((2 * n * H * D,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rec.process_complex_device(d_in.data_ptr(), code, n, pitch, d_out.data_ptr())
    rec.synchronize()
    X = d_out.cpu().numpy().view(np.complex64).reshape(n, H, D)
    assert np.isfinite(X.view(np.float32)).all()
    return X


def _device_pd(rec, dev, kw, pitch, off=(4, 8, 4), want=NAMES):
    """process_doppler_device on device frames into NaN-filled device memory, each output `off` bytes into its buffer; the words
    around the results and every unrequested buffer must stay NaN, after a refusal all of them."""
    import torch
    d_in, code, n, _ = dev
    pi, pr = dm.pair_shape(kw["axis"], kw["lag"], n, rec.cfg.height)
    D = rec.cfg.numdisplaypoints
    bins = pi * pr * D
    bufs = {w: torch.full(((2 if w == "corr" else 1) * bins + 4,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ptr = lambda w, o: bufs[w].data_ptr() + o if w in want else None   # noqa: E731
    try:
        rec.process_doppler_device(d_in.data_ptr(), code, n, pitch, kw["axis"], kw["lag"], ptr("phase", off[0]), ptr("corr", off[1]),
                                   ptr("power", off[2]), win=kw["win"], bulk=kw["bulk"], scale=kw["scale"], min_power=kw["min_power"])
    except FdoctError:
        rec.synchronize()
        for w in NAMES:
            assert np.isnan(bufs[w].cpu().numpy()).all(), w + ": written by a refused call"
        raise
    rec.synchronize()
    out = {}
    for i, w in enumerate(NAMES):
        flat = bufs[w].cpu().numpy()
        k, size = off[i] // 4, (2 if w == "corr" else 1) * bins
        if w in want:
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + size:]).all(), w + ": written outside the result"
            body = flat[k:k + size]
            out[w] = (body.view(np.complex64) if w == "corr" else body).reshape(pi, pr, D)
        else:
            assert np.isnan(flat).all(), w + ": written though not asked for"
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_device_frames_and_outputs_give_what_host_memory_gives(dtype):
    """Device frames whose rows are 4-byte aligned take the route host frames take and must give the host call's bits.  Rows 5
    samples apart are 205-byte rows of u8 and 410-byte rows of u16: the wave-per-row kernel reads 4-byte words and is out of
    scope there (fdoct_route_value.cpp: wave_scope), the chain runs generic_kernel, and the call is held to the composition on
    that route -- doppler() of process_complex_device on the same device frames -- which the aligned calls are held to as well."""
    W, M, N, D = cc.WAVE_SHAPE
    cfg = Config(width=W, height=cc.H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    raw = np.uint8 if dtype == np.uint8 else np.uint16
    frames = synth.make_frames(cc.FIRST_FRAME, cc.NF, W, cc.H, dtype=raw).astype(dtype)
    rec = _handle(cfg, synth.make_background(W, dtype=raw).astype(np.float64))
    try:
        for kw in (_kw(dm.ASCANS, True), _kw(dm.FRAMES, None, win=(4, 8))):
            name = "%s frames in device memory, axis %d" % (np.dtype(dtype).name, kw["axis"])
            host = _pd(rec, frames, kw)
            _ran(rec, "wave", name)
            want, _ = _composed(rec, frames, kw)
            _same(host, want, name + ": the host call")
            for pad, explicit in ((0, False), (0, True), (5, True)):      # pitch_bytes 0: the rows are contiguous
                dev = _device_frames(frames, pad)
                pitch = dev[3] if explicit else 0
                route = "wave" if dev[3] % 4 == 0 else "generic"
                what = "%s, rows %d samples apart, pitch_bytes %d" % (name, pad, pitch)
                got = _device_pd(rec, dev, kw, pitch)
                _ran(rec, route, what)
                X = _device_complex(rec, dev, pitch)
                _ran(rec, route, what)
                rc, want = _raw(rec, X, **kw)
                assert rc == 0, rec.lib.fdoct_last_error(rec.h)
                _same(got, want, what + ": against doppler of process_complex_device")
                if route == "wave":
                    _same(got, host, what + ": against the host call")
        kw = _kw(dm.ASCANS, True)
        dev = _device_frames(frames, 0)
        _same(_device_pd(rec, dev, kw, 0, want=("phase",)), _pd(rec, frames, kw), "out_phase alone")
        with pytest.raises(FdoctError) as e:   # out_corr 4 bytes off a pair: refused, and the helper finds every buffer untouched
            _device_pd(rec, dev, kw, 0, off=(0, 4, 0))
        assert e.value.code == -1 and "8 bytes" in str(e.value)
        _same(_device_pd(rec, dev, kw, dev[3]), _pd(rec, frames, kw), "after the refusal")
    finally:
        rec.close()


# ---- d. depth edges ------------------------------------------------------------------------------------------------------------------
EDGE_CASES = de.chain_depth_cases()


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c.name for c in EDGE_CASES])
def test_depths_around_one_tile(case):
    s = cc.edge_setup(case)
    rec = _handle(s.cfg, s.yb, **s.hkw)
    try:
        for kw in (_kw(dm.ASCANS, True), _kw(dm.FRAMES, None), _kw(dm.ASCANS, (0, 1), win=(4, 8))):
            what = "%s, axis %d, bulk %s" % (case.name, kw["axis"], kw["bulk"])
            got = _pd(rec, s.frames, kw)
            _ran(rec, case.route, what)
            want, _ = _composed(rec, s.frames, kw)
            _ran(rec, case.route, what)
            # (one depth with the bulk correction: B is the row's only term, T conj(B) / |B| is real and every angle is 0)
            _same(got, want, what, live=not (case.D == 1 and kw["bulk"]))
            assert got["phase"].shape == dm.pair_shape(kw["axis"], 1, cc.NF, cc.H) + (case.D,)
    finally:
        rec.close()


# ---- e. state ------------------------------------------------------------------------------------------------------------------------
def test_a_staged_handle_refuses_and_stays_staged():
    """C2's shape in the two-kernel mode: FDOCT_ERR_UNSUPPORTED as process_complex refuses it, the outputs untouched, and
    fdoct_process afterwards is staged still, with the same bits."""
    cfg = Config(width=2048, height=cc.H, numfftpoints=2048, numdisplaypoints=1024)
    frames = synth.make_frames(cc.FIRST_FRAME, cc.NF, 2048, cc.H)
    rec = _handle(cfg, synth.make_background(2048).astype(np.float64))
    try:
        rec.set_staged(True)
        before = rec.process(frames)
        assert rec.last_kernel() == capi.KERNEL_FUSED_STAGED
        rc, outs = _pd_raw(rec, frames, _kw(dm.ASCANS, True))
        assert rc == -2 and b"staged" in rec.lib.fdoct_last_error(rec.h), rec.lib.fdoct_last_error(rec.h)
        _untouched(outs)
        after = rec.process(frames)
        assert rec.last_kernel() == capi.KERNEL_FUSED_STAGED
    finally:
        rec.close()
    for a, b in zip(before, after):
        assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b))


def test_refusals_leave_poisoned_outputs_alone_and_the_handle_working():
    W, M, N, D = cc.WAVE_SHAPE
    cfg = Config(width=W, height=cc.H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    frames = synth.make_frames(cc.FIRST_FRAME, cc.NF, W, cc.H)
    kw = _kw(dm.ASCANS, True)
    bare = Reconstructor(cfg)                     # no background: FDOCT_ERR_STATE, on a handle that has run nothing
    try:
        rc, outs = _pd_raw(bare, frames, kw)
        assert rc == -5 and b"background" in bare.lib.fdoct_last_error(bare.h), bare.lib.fdoct_last_error(bare.h)
        _untouched(outs)
    finally:
        bare.close()
    rec = _handle(cfg, synth.make_background(W).astype(np.float64))
    try:
        for why, change in (("the frames axis with nframes == lag", dict(kw=dict(_kw(dm.FRAMES, True), lag=cc.NF))),
                            ("a pitch below a row", dict(pitch=2 * W - 2)), ("a bad dtype", dict(dtype=9)), ("no frames", dict(nframes=0))):
            rc, outs = _pd_raw(rec, frames, **dict(dict(kw=kw), **change))
            assert rc == -1, "%s: %d, %s" % (why, rc, rec.lib.fdoct_last_error(rec.h))
            _untouched(outs)
        rc, outs = _pd_raw(rec, frames, kw, want=())
        assert rc == -1 and b"no output" in rec.lib.fdoct_last_error(rec.h)
        got = _pd(rec, frames, kw)                # ... and the handle's first successful call comes after all of them
        _ran(rec, "wave", "after the refusals")
        want, _ = _composed(rec, frames, kw)
        _same(got, want, "after the refusals")
    finally:
        rec.close()


def test_a_clone_gives_its_parents_bits():
    W, M, N, D = cc.WAVE_SHAPE
    cfg = Config(width=W, height=cc.H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    frames = synth.make_frames(cc.FIRST_FRAME, cc.NF, W, cc.H)
    kw = _kw(dm.ASCANS, True)
    rec = _handle(cfg, synth.make_background(W).astype(np.float64))
    twin = None
    try:
        first = _pd(rec, frames, kw)              # the parent holds ws_cx, ws_dop_bulk and its compiled kernel when it is cloned
        twin = rec.clone_to_device(0)
        cloned = _pd(twin, frames, kw)            # the clone's first call
        _ran(twin, "wave", "the clone")
        _same(cloned, first, "the clone against its parent")
        second = _pd(rec, frames, kw)
        _ran(rec, "wave", "the parent after the clone's call")
        _same(second, first, "the parent after the clone's call")
        want, _ = _composed(twin, frames, kw)
        _same(cloned, want, "the clone against its own composition")
    finally:
        if twin is not None:
            twin.close()
        rec.close()
