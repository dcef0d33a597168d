"""GPU tests of the Doppler stage (include/fdoct_doppler.h; Reconstructor.doppler, process_doppler), held to tests/doppler_model.py
on the fields and cases of tests/doppler_cases.py: correlation and power against the composition in double by the project's
adjudication, the phase against the angle of the kernel's own written correlation, masked bins exactly 0; every subset of the
outputs the same bits as all three; NaN-poisoned outputs fully overwritten.  Then the invariants: device memory against host
memory, a batch taller than one pass of the capped grids against the base batch it repeats, alignment, refusals that leave poisoned
outputs alone; and fdoct_process_doppler against doppler() applied to what process_complex returns.  The ratios of every case
go to helpers.TRUTH_LOG."""
import itertools

import numpy as np
import pytest

import doppler_cases as dc
import doppler_model as dm
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

NAMES = ("phase", "corr", "power")


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=32))   # the stage reads nothing of the geometry
    yield r
    r.close()


def _poisoned(shape, name):
    if name == "corr":
        return np.full(shape, np.complex64(complex(np.nan, -7.0)), np.complex64)
    return np.full(shape, np.float32(np.nan), np.float32)


def _untouched(outs):
    for name, a in outs.items():
        v = a.view(np.float32)
        if name == "corr":
            v = v.reshape(-1, 2)
            assert np.isnan(v[:, 0]).all() and np.all(v[:, 1] == -7.0), name
        else:
            assert np.isnan(v).all(), name


def _raw(rec, X, want=NAMES, nframes=None, ascans=None, depths=None, params=None, **kw):
    """fdoct_doppler itself on host memory with poisoned outputs: (return code, dict of the outputs)."""
    n, H, D = X.shape
    p = params if params is not None else capi.doppler_params(kw["axis"], kw["lag"], kw.get("win", (1, 1)), kw.get("bulk"), kw.get("scale", 1.0),
                                                                kw.get("min_power", 0.0))
    shape = dm.pair_shape(kw["axis"], kw["lag"], n, H) + (D,) if params is None else (n, H, D)
    outs = {w: _poisoned(shape, w) for w in want}
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    rc = rec.lib.fdoct_doppler(rec.h, X.ctypes.data, capi.MEM_HOST, n if nframes is None else nframes, H if ascans is None else ascans,
                               D if depths is None else depths, p, ptr("phase"), ptr("corr"), ptr("power"), capi.MEM_HOST)
    return rc, outs


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", dc.CASES, ids=[c["what"] for c in dc.CASES])
def test_every_case_against_the_model(rec, case):
    X, kw = dc.case_field(case), dc.case_args(case)
    rc, full = _raw(rec, X, **kw)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    dm.check(full, X, kw["axis"], kw["lag"], case["what"], kw["win"], kw["bulk"], kw["scale"], kw["min_power"])   # (finite everywhere: no poison left)
    for k in (1, 2):
        for want in itertools.combinations(NAMES, k):
            rc, part = _raw(rec, X, want=want, **kw)
            assert rc == 0 and set(part) == set(want)
            for w in want:
                np.testing.assert_array_equal(_bits(part[w]), _bits(full[w]), err_msg="%s alone in %s" % (w, want))
    got = rec.doppler(X, **kw)   # the binding returns the same arrays
    for w, a in zip(NAMES, got):
        np.testing.assert_array_equal(_bits(a), _bits(full[w]))
    if case["zero_row"]:
        f, r = case["zero_row"]
        rows = [q for q in (r, r - kw["lag"]) if 0 <= q < full["corr"].shape[1]] if kw["axis"] == dm.ASCANS else [r]
        images = [f] if kw["axis"] == dm.ASCANS else [q for q in (f, f - kw["lag"]) if 0 <= q < full["corr"].shape[0]]
        if kw["win"] == (1, 1):
            assert np.all(full["corr"][images][:, rows] == 0) and np.all(full["phase"][images][:, rows] == 0)


def _device(rec, X, kw, off=(0, 0, 0), want=NAMES):
    """doppler_device on pairs in device memory into NaN-filled device memory, each output `off` bytes into its buffer."""
    import torch
    n, H, D = X.shape
    pi, pr = dm.pair_shape(kw["axis"], kw["lag"], n, H)
    bins = pi * pr * D
    d_in = torch.from_numpy(np.ascontiguousarray(X).view(np.float32).reshape(-1)).cuda()
    bufs = {w: torch.full(((2 if w == "corr" else 1) * bins + 4,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ptr = lambda w, o: bufs[w].data_ptr() + o if w in want else None   # noqa: E731
    rec.doppler_device(d_in.data_ptr(), n, H, D, kw["axis"], kw["lag"], ptr("phase", off[0]), ptr("corr", off[1]), ptr("power", off[2]),
                       win=kw["win"], bulk=kw["bulk"], scale=kw["scale"], min_power=kw["min_power"])
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
            assert np.isnan(flat).all()
    return out


@pytest.mark.parametrize("case", [dc.CASES[3], dc.CASES[12]], ids=lambda c: c["what"])
def test_device_memory_gives_what_host_memory_gives_and_alignment(rec, case):
    X, kw = dc.case_field(case), dc.case_args(case)
    rc, host = _raw(rec, X, **kw)
    assert rc == 0
    dev = _device(rec, X, kw, off=(4, 8, 4))   # out_phase and out_power 4-byte aligned only, out_corr 8-byte aligned only
    for w in NAMES:
        np.testing.assert_array_equal(_bits(dev[w]), _bits(host[w]), err_msg=w)
    with pytest.raises(FdoctError) as e:       # out_corr 4 bytes off a pair: refused, nothing written (the helper asserts that)
        _device(rec, X, kw, off=(0, 4, 0))
    assert e.value.code == -1 and "8 bytes" in str(e.value)


@pytest.mark.parametrize("axis", [dm.ASCANS, dm.FRAMES], ids=["A-scans", "frames"])
def test_a_batch_beyond_one_pass_of_the_grids_repeats_its_base_bit_for_bit(rec, axis):
    """Frames of 13 x 67 with the bulk correction on, so that both kernels loop: the tall batch's frame f is the base's frame
    f mod 3, and pair image p of the tall result equals pair image p mod 3 of the base's, bit for bit."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    base_n, lag = dc.TALL_BASE[axis]
    n = dc.tall_frames(axis, cus)
    assert dc.tall_ok(axis, n, cus) and dc.base_ok(axis, cus)
    three = dc.field(3, dc.TALL_H, dc.TALL_D, 50, speckle=True)
    kw = dict(axis=axis, lag=lag, win=(3, 5), bulk=True, scale=1.0, min_power=0.0)
    base = np.ascontiguousarray(three[np.arange(base_n) % 3])
    rc, want = _raw(rec, base, **kw)
    assert rc == 0
    dm.check(want, base, axis, lag, "tall batch's base, axis %d" % axis, (3, 5), True)
    tall = np.ascontiguousarray(three[np.arange(n) % 3])
    got = _device(rec, tall, kw)
    pi = dm.pair_shape(axis, lag, n, dc.TALL_H)[0]
    for w in NAMES:
        np.testing.assert_array_equal(_bits(got[w]), _bits(want[w][np.arange(pi) % 3]), err_msg="%s, %d frames on %d CUs" % (w, n, cus))


def test_refusals_leave_poisoned_outputs_alone(rec):
    X = dc.field(2, 12, 20, 60)
    good = dict(axis=dm.ASCANS, lag=1, win=(3, 5), bulk=None, scale=1.0, min_power=0.0)
    bad = [dict(win=(0, 5)), dict(win=(3, 33)), dict(win=(33, 1)), dict(lag=0), dict(lag=-1), dict(lag=12), dict(axis=dm.FRAMES, lag=2), dict(axis=2),
           dict(bulk=(20, 0)), dict(bulk=(-1, 4)), dict(bulk=(10, 11)), dict(bulk=(0, -1)), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(min_power=float("nan")), dict(min_power=-1.0), dict(min_power=float("inf"))]
    for change in bad:
        kw = dict(good, **change)
        p = capi.doppler_params(kw["axis"], kw["lag"], kw["win"], kw["bulk"], kw["scale"], kw["min_power"])
        rc, outs = _raw(rec, X, params=p, axis=kw["axis"], lag=kw["lag"])
        assert rc == -1, change
        _untouched(outs)
    rc, outs = _raw(rec, X, want=(), **good)
    assert rc == -1 and b"no output" in rec.lib.fdoct_last_error(rec.h)
    for change in (dict(nframes=0), dict(ascans=1), dict(depths=0)):
        rc, outs = _raw(rec, X, **dict(good, **change))
        assert rc == -1, change
        _untouched(outs)
    p = capi.doppler_params(**good)
    outs = {w: _poisoned((2, 11, 20), w) for w in NAMES}
    lib, h = rec.lib, rec.h
    call = lambda x=X.ctypes.data, sp=0, pp=p, ph=outs["phase"].ctypes.data, co=outs["corr"].ctypes.data, pw=outs["power"].ctypes.data, osp=0: (   # noqa: E731
        lib.fdoct_doppler(h, x, sp, 2, 12, 20, pp, ph, co, pw, osp))
    assert call(x=None) == -1 and call(pp=None) == -1 and call(sp=7) == -1 and call(osp=-1) == -1
    assert call(x=X.ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(co=outs["corr"].ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(ph=outs["phase"].ctypes.data + 2) == -1 and call(pw=outs["power"].ctypes.data + 1) == -1
    assert call(pw=outs["phase"].ctypes.data + 8) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(co=X.ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    _untouched(outs)
    assert call() == 0   # ... and the handle works afterwards
    with pytest.raises(FdoctError):
        rec.doppler(X, dm.ASCANS, 1, want=("phase", "phase"))
    with pytest.raises(FdoctError):
        rec.doppler(X.astype(np.complex128), dm.ASCANS, 1)


# ---- end to end: camera frames -> chain -> stage --------------------------------------------------------------------------------
E2E = [("200 x4 -> 2560, D 320", 200, 4, 2560, 320), ("2048 -> 2048, D 1024", 2048, 1, 2048, 1024)]


@pytest.mark.parametrize("shape", E2E, ids=[s[0] for s in E2E])
def test_process_doppler_is_doppler_of_process_complex(shape):
    what, W, M, N, D = shape
    cfg = Config(width=W, height=12, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    r = Reconstructor(cfg)
    r.set_background(synth.make_background(W).astype(np.float64))
    frames = synth.make_frames(4, 2, W, 12, dtype=np.uint16)
    fused = N == 2048
    before = r.process(frames) if fused else None
    if fused:
        assert r.last_kernel() == capi.KERNEL_FUSED
    X = r.process_complex(frames)
    family = r.last_kernel()
    assert family in (capi.KERNEL_WAVE_JIT, capi.KERNEL_GENERIC)
    for kw in (dict(axis=dm.ASCANS, lag=1, win=(3, 5), bulk=True, scale=2.0, min_power=float(np.float32(np.median(np.abs(X) ** 2)))),
               dict(axis=dm.FRAMES, lag=1, win=(4, 8))):
        want = r.doppler(X, **kw)
        got = r.process_doppler(frames, **kw)
        assert r.last_kernel() == family
        for w, a, b in zip(NAMES, got, want):
            assert np.isfinite(a.view(np.float32)).all()
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="%s: %s" % (what, w))
        assert np.count_nonzero(got[0]) > 0
    only = r.process_doppler(frames, dm.ASCANS, 1, win=(3, 5), want="phase")
    assert only.dtype == np.float32 and only.shape == (2, 11, D)
    if fused:   # the fused handle runs the fused kernel afterwards, with the same bits
        after = r.process(frames)
        assert r.last_kernel() == capi.KERNEL_FUSED
        for a, b in zip(before, after):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    # averages = 2 is refused as process_complex refuses it, with the outputs untouched
    r.set_averages(2)
    p = capi.doppler_params(dm.ASCANS, 1, (3, 5))
    outs = {w: _poisoned((2, 11, D), w) for w in NAMES}
    rc = r.lib.fdoct_process_doppler(r.h, frames.ctypes.data, capi.DTYPE_U16, capi.MEM_HOST, 2, 0, p, outs["phase"].ctypes.data,
                                     outs["corr"].ctypes.data, outs["power"].ctypes.data, capi.MEM_HOST)
    assert rc == -2 and b"averages" in r.lib.fdoct_last_error(r.h)
    _untouched(outs)
    with pytest.raises(FdoctError) as e:
        r.process_doppler(frames, dm.ASCANS, 1)
    assert e.value.code == -2
    r.close()
