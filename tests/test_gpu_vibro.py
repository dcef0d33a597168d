"""GPU tests of the vibrometry stage (include/fdoct_vibro.h; fdoct_amd/vibrometry.py), held to tests/vibro_model.py on the
catalogue of tests/vibro_cases.py: every case against the truth by the project's adjudication; a vibration of known amplitude and
phase against its closed form; bit-identity across subsets of outputs, runs, memory spaces and the contents of other pixels; a
NaN's reach; the chain form on both complex kernel families; every refusal on poisoned outputs; stream order behind a stall."""
import itertools

import numpy as np
import pytest

import stream_stall as ss
import vibro_cases as vc
import vibro_model as vm
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth, vibrometry

pytestmark = pytest.mark.gpu

NAMES = vibrometry.WANTS
IDS = [c["what"] for c in vc.CASES]


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage alone reads nothing of the geometry
    yield r
    r.close()


def _shapes(nf, H, D):
    return {"amp": ((nf, H, D), np.complex64), "rms": ((H, D), np.float32), "drift": ((H, D), np.float32), "power": ((H, D), np.float32)}


def _poisoned(nf, H, D, want=NAMES):
    out = {}
    for w in want:
        shape, dt = _shapes(nf, H, D)[w]
        out[w] = np.full(shape, complex(np.nan, np.nan) if dt == np.complex64 else np.nan, dt)
    return out


def _untouched(outs):
    for w, a in outs.items():
        assert np.isnan(a.view(np.float32)).all(), w + " was written by a refused call"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def _same(a, b, what=""):
    for w in a:
        np.testing.assert_array_equal(_bits(a[w]), _bits(b[w]), err_msg="%s: %s" % (what, w))


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=IDS)
def test_every_case_against_the_model(rec, i):
    c = vc.CASES[i]
    X, refs = vc.case_refs(i)
    p = vibrometry.params(**vc.case_params(c))
    info = vibrometry.plan(p, c["T"], c["H"], c["D"])
    assert info["chunks"] == vc.chunks(c["T"], c["H"], c["D"], c["chunk_steps"])
    got = vibrometry.vibro(rec, X, p)
    assert set(got) == set(NAMES if c["freq"] else NAMES[1:])
    vm.check(got, X, c["what"], refs=refs, **vc.case_args(c))


def test_the_reference_removes_what_the_call_without_it_keeps(rec):
    i, j = (IDS.index("T 40, 4 x 130, common mode of +-3 rad, %s" % s) for s in ("reference", "no reference"))
    X, _ = vc.case_refs(i)
    a = vibrometry.vibro(rec, X, vibrometry.params(**vc.case_params(vc.CASES[i])))
    b = vibrometry.vibro(rec, X, vibrometry.params(**vc.case_params(vc.CASES[j])))
    live = np.ones(130, bool)
    live[60:68] = False
    assert np.median(a["rms"][:, live]) < 1.0 < np.median(b["rms"][:, live])
    assert np.abs(a["amp"] - b["amp"])[0][:, live].max() > 0.1


def test_a_vibration_of_known_amplitude_and_phase(rec):
    """phi(t) = a sin(2 pi nu t + psi), nu = k / T.  The stage measures phi from its first value and removes the mean; over whole
    cycles the mean of phi is 0, so phi' = phi, and
        A = (2 / T) sum_t a sin(x_t + psi) e^(-i x_t) = (a / (i T)) (T e^(i psi) - e^(-i psi) sum_t e^(-2 i x_t)) = -i a e^(i psi)
        rms = a sqrt(mean sin^2) = a / sqrt(2)
    (x_t = 2 pi k t / T; the sums of e^(-2 i x_t) and of cos(2 x_t + 2 psi) over t vanish because 2 k is no multiple of T)."""
    T, H, D, k = 64, 3, 67, 2
    nu = k / T
    rng = np.random.default_rng(77)
    a, psi = rng.uniform(0.0, 5.0, (H, D)), rng.uniform(-np.pi, np.pi, (H, D))
    a[0, 0], a[0, 1] = 5.0, 0.0
    assert a.max() * 2 * np.pi * nu < 1.0
    amp = 900.0 * (0.35 + rng.rayleigh(0.8, (H, D)))                 # static speckle
    static = rng.uniform(-np.pi, np.pi, (H, D))
    t = np.arange(T, dtype=np.float64)[:, None, None]
    X = (amp[None] * np.exp(1j * (static[None] + a[None] * np.sin(2 * np.pi * nu * t + psi[None])))).astype(np.complex64)
    kw = dict(freq=(nu,))
    got = vibrometry.vibro(rec, X, vibrometry.params(**kw))
    tol = vm.tolerances(X, **kw)
    ill, _ = vm.exemptions(X, tol=tol, **kw)
    assert not ill.any()
    # X is rounded to float pairs: a sample's angle moves by up to u sqrt(2), which E[t] -- 1.7e-6 a step -- covers from the first step on
    ra = float((np.abs(got["amp"][0] - (-1j) * a * np.exp(1j * psi)) / tol["amp"]).max())
    rr = float((np.abs(got["rms"] - a / np.sqrt(2.0)) / tol["rms"]).max())
    rd = float((np.abs(got["drift"] - a * (np.sin(2 * np.pi * nu * (T - 1) + psi) - np.sin(psi))) / tol["drift"]).max())
    print("known vibration: |amp + i a e^(i psi)| / tol = %.4f, |rms - a / sqrt 2| / tol = %.4f, drift %.4f" % (ra, rr, rd))
    assert ra <= 1.0 and rr <= 1.0 and rd <= 1.0
    assert abs(abs(got["amp"][0, 0, 0]) - 5.0) < 1e-4 and abs(got["amp"][0, 0, 1]) < 1e-4


DET = dict(freq=(vc.NU0, 0.5), ref=(10, 4), detrend=1, window=vm.HANN, scale=-2.0, min_power=1.3e6, chunk_steps=4)


def _det_field():
    return vc.field(16, 8, 130, 28, surface=(10, 4), common=1.5)


def test_subsets_runs_and_other_pixels_do_not_change_a_bit(rec):
    X = _det_field()
    p = vibrometry.params(**DET)
    full = vibrometry.vibro(rec, X, p)
    _same(full, vibrometry.vibro(rec, X, p), "a second run")
    assert np.count_nonzero(full["rms"]) > 0 and np.count_nonzero(full["rms"] == 0) > 0
    for n in (1, 2, 3):
        for want in itertools.combinations(NAMES, n):
            got = vibrometry.vibro(rec, X, p, want=want)
            _same(got, {w: full[w] for w in want}, "subset %s" % (want,))
    one = vibrometry.vibro(rec, X, dict(DET, chunk_steps=15))   # (one chunk: the series pass finishes the pixel itself)
    _same({w: one[w] for w in ("rms",)}, vibrometry.vibro(rec, X, dict(DET, chunk_steps=15), want=("rms",)), "subset, one chunk")
    # every pixel but one, outside the reference range, replaced by noise: that pixel and the reference bins keep their bits
    rng = np.random.default_rng(5)
    Y = (rng.normal(0, 3000, X.shape) + 1j * rng.normal(0, 3000, X.shape)).astype(np.complex64)
    Y[:, :, 10:14] = X[:, :, 10:14]
    Y[:, 5, 77] = X[:, 5, 77]
    other = vibrometry.vibro(rec, Y, p)
    for w in NAMES:
        np.testing.assert_array_equal(_bits(other[w][..., 5, 77]), _bits(full[w][..., 5, 77]), err_msg=w)
        np.testing.assert_array_equal(_bits(other[w][..., :, 10:14]), _bits(full[w][..., :, 10:14]), err_msg=w)
    assert not np.array_equal(_bits(other["rms"]), _bits(full["rms"]))


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_nan_reaches_its_own_pixel_or_a_scan_only(rec, bad):
    X = _det_field()
    kw = dict(DET, min_power=0.0)
    clean = vibrometry.vibro(rec, X, kw)
    Y = X.copy()
    Y[7, 3, 99] = bad                      # a pixel outside the reference range, in the second chunk
    got = vibrometry.vibro(rec, Y, kw)
    hit = np.zeros((8, 130), bool)
    hit[3, 99] = True
    for w in NAMES:
        np.testing.assert_array_equal(_bits(got[w][..., ~hit]), _bits(clean[w][..., ~hit]), err_msg=w)
        assert not np.isfinite(_f32(got[w][..., hit])).all(), w
    Z = X.copy()
    Z[2, 6, 11] = bad                      # in the reference range of A-scan 6
    got = vibrometry.vibro(rec, Z, kw)
    row = np.zeros((8, 130), bool)
    row[6] = True
    for w in NAMES:
        np.testing.assert_array_equal(_bits(got[w][..., ~row]), _bits(clean[w][..., ~row]), err_msg=w)
    for w in ("amp", "rms", "drift"):
        assert np.isnan(_f32(got[w][..., row])).all(), w
    only = np.zeros((8, 130), bool)
    only[6, 11] = True
    np.testing.assert_array_equal(_bits(got["power"][~only]), _bits(clean["power"][~only]))


def _busy_stream():
    """The caller's stream of the stalled runs: a high-priority one.  torch hands out the streams of its default pool in turn, and
    which two of them a later test gets decides whether they share a hardware queue (tests/test_gpu_stream_order.py's teeth check
    needs two that do not); taking from the other pool leaves that turn where it was."""
    import torch
    return torch.cuda.Stream(priority=-1)


def _sizes(nf, H, D):
    return {"amp": nf * H * D * 8, "rms": H * D * 4, "drift": H * D * 4, "power": H * D * 4}


def _device_outputs(bufs, sizes, want, off, nf, H, D):
    out = {}
    for w in NAMES:
        flat = bufs[w].cpu().numpy()
        k, size = off // 4, sizes[w] // 4
        if w in want:
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + size:]).all(), w + ": written outside the result"
            body = flat[k:k + size].copy()
            shape, dt = _shapes(nf, H, D)[w]
            out[w] = body.view(dt).reshape(shape)
        else:
            assert np.isnan(flat).all(), w + ": written though not asked for"
    return out


def _device(rec, X, kw, want=NAMES, off=0, fill_on=None):
    """vibro_device on pairs in device memory into NaN-filled device memory, every output `off` bytes into its buffer."""
    import torch
    T, H, D = X.shape
    nf = len(kw.get("freq", ()))
    sizes = _sizes(nf, H, D)
    src = torch.from_numpy(np.ascontiguousarray(X).view(np.float32).reshape(-1).copy()).cuda()
    d_in = torch.zeros_like(src) if fill_on is not None else src
    bufs = {w: torch.full((sizes[w] // 4 + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:   # the input arrives on the busy stream, behind the stall
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    ptr = lambda w: bufs[w].data_ptr() + off if w in want else None   # noqa: E731
    vibrometry.vibro_device(rec, d_in.data_ptr(), T, H, D, kw, ptr("amp"), ptr("rms"), ptr("drift"), ptr("power"))
    if ev is not None:
        ss.still_running(ev, "vibro_device")
        fill_on.synchronize()
    rec.synchronize()
    return _device_outputs(bufs, sizes, want, off, nf, H, D)


@pytest.mark.parametrize("kw", [DET, dict(DET, chunk_steps=15), dict(freq=(), detrend=0)], ids=["four chunks", "one chunk", "no frequency"])
def test_device_memory_gives_what_host_memory_gives(rec, kw):
    X = _det_field()[:, :3, :67] if not kw.get("ref") else _det_field()
    names = NAMES if kw["freq"] else NAMES[1:]
    host = vibrometry.vibro(rec, X, kw)
    dev = _device(rec, X, kw, want=names, off=8)
    _same(dev, host, "device memory")
    part = _device(rec, X, kw, want=("drift",), off=4)
    _same(part, {"drift": host["drift"]}, "device memory, one output")


def test_refusals_leave_poisoned_outputs_alone(rec):
    lib, h = rec.lib, rec.h
    T, H, D = 6, 3, 20
    X = vc.field(T, H, D, 3)
    outs = _poisoned(2, H, D)
    good = dict(freq=(0.1, 0.5), ref=(2, 3))

    def call(x=X.ctypes.data, space=capi.MEM_HOST, out_space=capi.MEM_HOST, T=T, H=H, D=D, p=None, nop=False, **o):
        p = vibrometry.params(**good) if p is None else p
        ptr = {w: outs[w].ctypes.data for w in NAMES}
        ptr.update(o)
        return lib.fdoct_vibro(h, x, space, T, H, D, None if nop else p, ptr["amp"], ptr["rms"], ptr["drift"], ptr["power"], out_space)

    def P(**kw):
        return vibrometry.params(**dict(good, **kw))

    assert call(x=None) == -1 and call(nop=True) == -1 and call(space=7) == -1 and call(out_space=-1) == -1
    assert call(T=1) == -1 and call(T=65537) == -1 and call(T=0) == -1
    assert call(H=0) == -1 and call(D=0) == -1 and call(H=-3) == -1 and call(H=1 << 20, D=17) == -1 and call(H=1 << 16, D=1 << 16) == -1
    p9 = P()
    p9.nfreq = 9
    pm = P()
    pm.nfreq = -1
    assert call(p=p9) == -1 and call(p=pm) == -1
    for f in (0.0, -0.1, 0.5000001, float("nan"), float("inf")):
        assert call(p=P(freq=(0.1, f))) == -1 and b"(0, 0.5]" in lib.fdoct_last_error(h), f
    for r in ((-1, 2), (20, 1), (0, 21), (19, 2), (3, -1)):
        assert call(p=P(ref=r)) == -1 and b"reference range" in lib.fdoct_last_error(h), r
    pr = P()
    pr.ref = 2
    assert call(p=pr) == -1
    assert call(p=P(detrend=2)) == -1 and call(p=P(detrend=-1)) == -1 and call(p=P(window=2)) == -1 and call(p=P(window=-1)) == -1
    for kw in (dict(scale=float("nan")), dict(scale=float("inf")), dict(min_power=float("nan")), dict(min_power=float("inf")), dict(min_power=-1.0),
               dict(chunk_steps=-1)):
        assert call(p=P(**kw)) == -1, kw
    assert call(amp=None, rms=None, drift=None, power=None) == -1 and b"no output" in lib.fdoct_last_error(h)
    assert call(p=P(freq=())) == -1 and b"nfreq 0" in lib.fdoct_last_error(h)
    assert call(x=X.ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(amp=outs["amp"].ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(rms=outs["rms"].ctypes.data + 2) == -1 and call(drift=outs["drift"].ctypes.data + 1) == -1 and call(power=outs["power"].ctypes.data + 3) == -1
    assert call(power=outs["rms"].ctypes.data + 8) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(drift=outs["amp"].ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(rms=X.ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    _untouched(outs)
    assert np.array_equal(X, vc.field(T, H, D, 3))
    assert call() == 0   # ... and the handle works afterwards
    assert all(np.isfinite(a.view(np.float32)).all() for a in outs.values())
    with pytest.raises(FdoctError):
        vibrometry.vibro(rec, X, good, want=("rms", "rms"))
    with pytest.raises(FdoctError):
        vibrometry.vibro(rec, X.astype(np.complex128), good)


# ---- end to end: camera frames -> chain -> stage --------------------------------------------------------------------------------
CHAIN_KW = dict(freq=(0.25, 0.1), ref=(40, 8), detrend=1, window=vm.HANN, scale=0.5, chunk_steps=2)
W, H, M, N, D, T = 200, 6, 4, 2560, 320, 6


def _chain_handle(jit):
    r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M))
    r.set_background(synth.make_background(W).astype(np.float64))
    if not jit:
        r.set_jit(False)
    return r


@pytest.mark.parametrize("jit", [True, False], ids=["wave, run-time compiled", "workgroup per row"])
def test_process_vibro_is_vibro_of_process_complex(jit):
    r = _chain_handle(jit)
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    X = r.process_complex(frames)
    family = r.last_kernel()
    assert family == (capi.KERNEL_WAVE_JIT if jit else capi.KERNEL_GENERIC), r.jit_note()
    assert X.shape == (T, H, D)
    min_power = float(np.float32(np.median(np.abs(X) ** 2)))
    for kw in (dict(CHAIN_KW, min_power=min_power), dict(freq=(), chunk_steps=0)):
        want = vibrometry.vibro(r, X, kw)
        got = vibrometry.process_vibro(r, frames, kw)
        assert r.last_kernel() == family
        _same(got, want, "the chain form")
        assert all(np.isfinite(a.view(np.float32)).all() for a in got.values()) and np.count_nonzero(got["rms"]) > 0
    only = vibrometry.process_vibro(r, frames, CHAIN_KW, want="drift")
    assert only.dtype == np.float32 and only.shape == (H, D)
    assert r.process_complex(frames).tobytes() == X.tobytes()   # the stage changed nothing a later call reads
    # averages = 2 is refused as process_complex refuses it, with the outputs untouched; so is a single frame, by the stage
    outs = _poisoned(2, H, D)
    p = vibrometry.params(**CHAIN_KW)
    args = (p, outs["amp"].ctypes.data, outs["rms"].ctypes.data, outs["drift"].ctypes.data, outs["power"].ctypes.data, capi.MEM_HOST)
    assert r.lib.fdoct_process_vibro(r.h, frames.ctypes.data, capi.DTYPE_U16, capi.MEM_HOST, 1, 0, *args) == -1
    r.set_averages(2)
    assert r.lib.fdoct_process_vibro(r.h, frames.ctypes.data, capi.DTYPE_U16, capi.MEM_HOST, T, 0, *args) == -2
    assert b"averages" in r.lib.fdoct_last_error(r.h)
    _untouched(outs)
    r.close()


def test_vibro_device_behind_a_stall_matches_a_quiet_run_on_a_second_handle(rec):
    X = _det_field()
    second = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))
    quiet = _device(second, X, DET)
    second.close()
    _device(rec, X, DET)   # the warm call: every workspace has its size
    S = _busy_stream()
    rec.set_stream(S.cuda_stream)
    try:
        busy = _device(rec, X, DET, fill_on=S)
    finally:
        S.synchronize()
        rec.set_stream(None)
    _same(busy, quiet, "behind a stall")
    assert np.count_nonzero(quiet["rms"]) > 0


def _process_device(r, frames, kw, fill_on=None):
    import torch
    nf = len(kw["freq"])
    sizes = _sizes(nf, H, D)
    src = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()
    d_in = torch.zeros_like(src) if fill_on is not None else src
    bufs = {w: torch.full((sizes[w] // 4 + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    vibrometry.process_vibro_device(r, d_in.data_ptr(), capi.DTYPE_U16, frames.shape[0], W * 2, kw, bufs["amp"].data_ptr(), bufs["rms"].data_ptr(),
                                    bufs["drift"].data_ptr(), bufs["power"].data_ptr())
    if ev is not None:
        ss.still_running(ev, "process_vibro_device")
        fill_on.synchronize()
    r.synchronize()
    return _device_outputs(bufs, sizes, NAMES, 0, nf, H, D)


def test_process_vibro_device_behind_a_stall_matches_a_quiet_run_on_a_second_handle():
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    second = _chain_handle(True)
    host = vibrometry.process_vibro(second, frames, CHAIN_KW)
    quiet = _process_device(second, frames, CHAIN_KW)
    second.close()
    _same(quiet, host, "device memory, the chain form")
    r = _chain_handle(True)
    _process_device(r, frames, CHAIN_KW)   # the warm call: the run-time compile, every workspace
    S = _busy_stream()
    r.set_stream(S.cuda_stream)
    try:
        busy = _process_device(r, frames, CHAIN_KW, fill_on=S)
    finally:
        S.synchronize()
        r.set_stream(None)
    r.close()
    _same(busy, quiet, "the chain form behind a stall")
