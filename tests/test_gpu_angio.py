"""GPU tests of the angiography stage (include/fdoct_angio.h; fdoct_amd/angiography.py), held to tests/angio_model.py on the
catalogue of tests/angio_cases.py: every case against the truth by the project's adjudication, in both memory spaces on each side;
the tile seams; a group's isolation from its neighbours and from its place in the call, beyond one pass of the capped grid;
bit-identity across subsets of outputs and runs; every refusal on poisoned outputs; the chain form on all three complex kernel
families; stream order behind a stall."""
import itertools

import numpy as np
import pytest

import angio_cases as ac
import angio_model as am
import stream_stall as ss
from fdoct_amd import Config, FdoctError, Reconstructor, angiography, capi, synth

pytestmark = pytest.mark.gpu

NAMES = angiography.WANTS
IDS = [c["what"] for c in ac.CASES]
HOST, DEV = capi.MEM_HOST, capi.MEM_DEVICE


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage alone reads nothing of the geometry
    yield r
    r.close()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what=""):
    assert set(a) == set(b), (what, set(a), set(b))
    for w in a:
        np.testing.assert_array_equal(_bits(a[w]), _bits(b[w]), err_msg="%s: %s" % (what, w))


def _poisoned(G, H, D, want=NAMES):
    return {w: np.full((G, H, D), np.nan, np.float32) for w in want}


def _untouched(outs):
    for w, a in outs.items():
        assert np.isnan(a).all(), w + " was written by a refused call"


def _busy_stream():
    """The caller's stream of the stalled runs: a high-priority one, so that torch's default pool keeps its turn (tests/test_gpu_vibro.py)."""
    import torch
    return torch.cuda.Stream(priority=-1)


def _run(rec, X, kw, in_space=HOST, out_space=HOST, want=NAMES, off=0, fill_on=None):
    """fdoct_angio on pairs in `in_space` into NaN-filled buffers in `out_space`, every output `off` bytes into its buffer; what was
    asked for comes back, and nothing else was written.  fill_on: the input arrives on that stream, behind a stall."""
    import torch
    X = np.ascontiguousarray(X)
    T, H, D = X.shape
    p = angiography.params(**kw)
    G = T // p.repeats
    n = G * H * D
    keep = []
    if in_space == DEV:
        src = torch.from_numpy(X.view(np.float32).reshape(-1).copy()).cuda()
        d_in = torch.zeros_like(src) if fill_on is not None else src
        keep += [src, d_in]
        in_ptr = d_in.data_ptr()
    else:
        assert fill_on is None
        in_ptr = X.ctypes.data
    if out_space == DEV:
        bufs = {w: torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
        base = {w: bufs[w].data_ptr() for w in NAMES}
    else:
        bufs = {w: np.full(n + 8, np.nan, np.float32) for w in NAMES}
        base = {w: bufs[w].ctypes.data for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    ptr = lambda w: base[w] + off if w in want else None   # noqa: E731
    rec._check(rec.lib.fdoct_angio(rec.h, in_ptr, in_space, T, H, D, p, ptr("var"), ptr("decorr"), ptr("cdecorr"), ptr("power"), out_space))
    if ev is not None:
        ss.still_running(ev, "angio_device")
        fill_on.synchronize()
    rec.synchronize()
    return _collect(bufs, want, off, (G, H, D))


def _collect(bufs, want, off, shape):
    out, k, n = {}, off // 4, int(np.prod(shape))
    for w in NAMES:
        flat = bufs[w] if isinstance(bufs[w], np.ndarray) else bufs[w].cpu().numpy()
        if w in want:
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + n:]).all(), w + ": written outside the result"
            out[w] = flat[k:k + n].copy().reshape(shape)
        else:
            assert np.isnan(flat).all(), w + ": written though not asked for"
    return out


@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=IDS)
def test_every_case_against_the_model_in_both_memory_spaces(rec, i):
    c = ac.CASES[i]
    X, refs = ac.case_refs(i)
    kw = ac.case_args(c)
    info = angiography.plan(kw, X.shape[0], c["H"], c["D"])
    assert info["groups"] == c["groups"] and info["tiles"] == am.geometry(X.shape[0], c["repeats"], c["H"], c["D"])[1]
    got = angiography.angio(rec, X, kw)
    assert set(got) == set(NAMES) and all(a.shape == (c["groups"], c["H"], c["D"]) for a in got.values())
    am.check(got, X, c["what"], refs=refs, **kw)
    for ins, outs in ((HOST, HOST), (DEV, DEV), (HOST, DEV), (DEV, HOST)):
        _same(_run(rec, X, kw, ins, outs, off=4 if outs == DEV else 0), got, "memory spaces %d -> %d" % (ins, outs))


def test_the_catalogue_holds_the_tile_seams():
    for what in ("static, N 4, 2 groups of 17 x 65, window 3 x 5", "vessel, N 3, 16 x 64 exactly, window 3 x 5", "vessel, N 3, 1 x 130, window 3 x 5, bulk",
                 "independent, N 3, 33 x 1, window 5 x 3", "independent, N 3, 2 groups of 2 x 3, window 16 x 16", "vessel, N 2, 17 x 65, window 3 x 5"):
        assert what in IDS


ISO = dict(repeats=3, win=(3, 5), bulk=True, min_power=1.0e6)     # the fields' mean power: about half the pixels are masked


@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan", "1e30"])
def test_a_group_does_not_read_its_neighbours(rec, fill):
    mid = ac.field(1, 3, 17, 65, 31, kind="vessel")
    alone = angiography.angio(rec, mid, ISO)
    assert np.count_nonzero(alone["decorr"]) > 0 and np.count_nonzero(alone["decorr"] == 0) > 0      # the mask takes part
    X = np.full((9, 17, 65), complex(fill, fill), np.complex64)
    X[3:6] = mid
    got = angiography.angio(rec, X, ISO)
    _same({w: got[w][1:2] for w in NAMES}, alone, "the middle group")
    assert not np.isfinite(got["power"][0]).any() and not np.isfinite(got["power"][2]).any()    # (1e30 squared is no float)


@pytest.mark.parametrize("win", [(1, 1), (3, 3), (9, 9)], ids=["window 1 x 1 (4 staged pixels a thread)", "window 3 x 3 (6)", "window 9 x 9 (10)"])
def test_a_groups_place_in_the_call_does_not_change_a_bit(rec, win):
    cus = _cus()
    G = ac.placement_groups(cus)
    kw = dict(repeats=2, win=win, bulk=(1, 2))
    tiles = angiography.plan(kw, 2 * G, 2, 3)["tiles"]
    assert tiles == G and ac.beyond(tiles, ac.resident(cus)), (tiles, cus)     # one tile a group: more than one pass of the capped grid
    X = ac.field(G, 2, 2, 3, 41, kind="independent")
    X[-2:] = X[:2]
    got = angiography.angio(rec, X, kw)
    _same({w: got[w][-1] for w in NAMES}, {w: got[w][0] for w in NAMES}, "the group at index 0 and at the last index")
    one = angiography.angio(rec, X[:2], kw)
    _same({w: got[w][:1] for w in NAMES}, one, "the group alone")
    mid = ac.resident(cus) + 5                                                     # a group of the second pass, against the model
    ref = am.model(X[2 * mid:2 * mid + 2], truth=True, **kw)
    tol = am.tolerances(X[2 * mid:2 * mid + 2], **kw)
    for w in NAMES:
        assert np.all(np.abs(got[w][mid] - ref[w][0]) <= tol[w][0]), w


SUB = dict(repeats=4, win=(5, 5), bulk=(3, 40), min_power=1.0e6)


def test_subsets_and_runs_do_not_change_a_bit(rec):
    X = ac.field(2, 4, 17, 65, 51, kind="vessel")
    full = angiography.angio(rec, X, SUB)
    _same(full, angiography.angio(rec, X, SUB), "a second run")
    assert np.count_nonzero(full["cdecorr"]) > 0 and np.count_nonzero(full["cdecorr"] == 0) > 0
    for n in (1, 2, 3):
        for want in itertools.combinations(NAMES, n):
            _same(angiography.angio(rec, X, SUB, want=want), {w: full[w] for w in want}, "subset %s" % (want,))
    dev = _run(rec, X, SUB, DEV, DEV, want=("cdecorr",), off=4)
    _same(dev, {"cdecorr": full["cdecorr"]}, "device memory, one output")
    only = angiography.angio(rec, X, SUB, want="var")
    assert only.dtype == np.float32 and np.array_equal(_bits(only), _bits(full["var"]))
    # without the mask too, where nothing but an output's own sums is computed
    kw = dict(SUB, min_power=0.0, win=(1, 1))
    full = angiography.angio(rec, X, kw)
    for w in NAMES:
        _same(angiography.angio(rec, X, kw, want=(w,)), {w: full[w]}, "alone, no mask")


def test_refusals_leave_poisoned_outputs_alone(rec):
    lib, h = rec.lib, rec.h
    T, H, D = 6, 3, 20
    X = ac.field(2, 3, H, D, 61)
    Xpad = np.zeros(X.size + 1, np.complex64)
    outs = _poisoned(2, H, D)
    good = dict(repeats=3, win=(3, 5), bulk=(2, 3))

    def call(x=X.ctypes.data, space=HOST, out_space=HOST, T=T, H=H, D=D, p=None, nop=False, **o):
        p = angiography.params(**good) if p is None else p
        ptr = {w: outs[w].ctypes.data for w in NAMES}
        ptr.update(o)
        return lib.fdoct_angio(h, x, space, T, H, D, None if nop else p, ptr["var"], ptr["decorr"], ptr["cdecorr"], ptr["power"], out_space)

    def P(**kw):
        return angiography.params(**dict(good, **kw))

    # the three the stage cannot show without a handle
    assert call(x=Xpad.ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(power=outs["var"].ctypes.data + 8) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(decorr=X.ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(T=5) == -1 and call(T=7) == -1 and b"multiple" in lib.fdoct_last_error(h)
    # ... and the rest of the header's list
    assert call(x=None) == -1 and call(nop=True) == -1 and call(space=7) == -1 and call(out_space=-1) == -1
    assert call(p=P(repeats=1)) == -1 and call(p=P(repeats=65)) == -1 and call(T=0) == -1 and call(T=65538) == -1
    assert call(H=0) == -1 and call(D=0) == -1 and call(H=1 << 20, D=17) == -1
    assert call(p=P(win=(0, 1))) == -1 and call(p=P(win=(1, 17))) == -1
    pb = P()
    pb.bulk = 2
    assert call(p=pb) == -1 and call(p=P(bulk=(20, 0))) == -1 and call(p=P(bulk=(19, 2))) == -1
    assert call(p=P(min_power=float("nan"))) == -1 and call(p=P(min_power=-1.0)) == -1
    assert call(var=None, decorr=None, cdecorr=None, power=None) == -1 and b"no output" in lib.fdoct_last_error(h)
    assert call(var=outs["var"].ctypes.data + 2) == -1 and call(cdecorr=outs["cdecorr"].ctypes.data + 1) == -1
    _untouched(outs)
    assert np.array_equal(X, ac.field(2, 3, H, D, 61))
    assert call() == 0   # ... and the handle works afterwards
    assert all(np.isfinite(a).all() for a in outs.values())
    with pytest.raises(FdoctError):
        angiography.angio(rec, X, good, want=("var", "var"))


# ---- end to end: camera frames -> chain -> stage --------------------------------------------------------------------------------
CHAIN_KW = dict(repeats=3, win=(3, 5), bulk=(40, 8))
H, M, N, D, T = 6, 4, 2560, 320, 6
# the smallest shapes of tests/complex_cases.py and tests/degenerate_cases.py: (width, run-time compilation, the family that must run).
# 160 x 4 is a shape of the wave-per-row kernel's built-in list; the complex call runs the form that stores the pairs, which is
# compiled at run time for every shape (complex_cases.wave_family), so its family is the run-time compiled one there too.
CHAIN = {"wave, a built-in shape": (160, True, capi.KERNEL_WAVE_JIT), "wave, run-time compiled": (200, True, capi.KERNEL_WAVE_JIT),
         "workgroup per row": (200, False, capi.KERNEL_GENERIC)}


def _chain_handle(W, jit, background=True):
    r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M))
    if background:
        r.set_background(synth.make_background(W).astype(np.float64))
    if not jit:
        r.set_jit(False)
    return r


@pytest.mark.parametrize("name", list(CHAIN), ids=list(CHAIN))
def test_process_angio_is_angio_of_process_complex(name):
    W, jit, family = CHAIN[name]
    r = _chain_handle(W, jit)
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    X = r.process_complex(frames)
    assert r.last_kernel() == family, r.jit_note()
    assert X.shape == (T, H, D)
    min_power = float(np.float32(np.median(np.abs(X) ** 2)))
    for kw in (dict(CHAIN_KW, min_power=min_power), dict(repeats=2)):
        want = angiography.angio(r, X, kw)
        got = angiography.process_angio(r, frames, kw)
        assert r.last_kernel() == family
        _same(got, want, "the chain form")
        assert all(np.isfinite(a).all() for a in got.values()) and np.count_nonzero(got["var"]) > 0
    only = angiography.process_angio(r, frames, CHAIN_KW, want="cdecorr")
    assert only.dtype == np.float32 and only.shape == (T // 3, H, D)
    assert r.process_complex(frames).tobytes() == X.tobytes()   # the stage changed nothing a later call reads
    # averages = 2 is refused as process_complex refuses it, a frame count off the repeats by the stage; the outputs stay untouched
    outs = _poisoned(2, H, D)
    p = angiography.params(**CHAIN_KW)
    args = (p, outs["var"].ctypes.data, outs["decorr"].ctypes.data, outs["cdecorr"].ctypes.data, outs["power"].ctypes.data, HOST)
    assert r.lib.fdoct_process_angio(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, 5, 0, *args) == -1
    r.set_averages(2)
    assert r.lib.fdoct_process_angio(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, *args) == -2
    assert b"averages" in r.lib.fdoct_last_error(r.h)
    _untouched(outs)
    r.close()


def test_process_angio_without_a_background_is_a_state_error():
    r = _chain_handle(200, True, background=False)
    frames = synth.make_frames(4, T, 200, H, dtype=np.uint16)
    outs = _poisoned(2, H, D)
    p = angiography.params(**CHAIN_KW)
    rc = r.lib.fdoct_process_angio(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, p, outs["var"].ctypes.data, outs["decorr"].ctypes.data,
                                   outs["cdecorr"].ctypes.data, outs["power"].ctypes.data, HOST)
    assert rc == -5, (rc, r.lib.fdoct_last_error(r.h))
    _untouched(outs)
    r.close()


def test_angio_device_behind_a_stall_matches_a_quiet_run_on_a_second_handle(rec):
    X = ac.field(2, 4, 17, 65, 51, kind="vessel")
    second = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))
    quiet = _run(second, X, SUB, DEV, DEV)
    second.close()
    _run(rec, X, SUB, DEV, DEV)   # the warm call: every workspace has its size
    S = _busy_stream()
    rec.set_stream(S.cuda_stream)
    try:
        busy = _run(rec, X, SUB, DEV, DEV, fill_on=S)
    finally:
        S.synchronize()
        rec.set_stream(None)
    _same(busy, quiet, "behind a stall")
    assert np.count_nonzero(quiet["cdecorr"]) > 0


def _process_device(r, frames, W, kw, fill_on=None):
    import torch
    G = frames.shape[0] // kw["repeats"]
    n = G * H * D
    src = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()
    d_in = torch.zeros_like(src) if fill_on is not None else src
    bufs = {w: torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    angiography.process_angio_device(r, d_in.data_ptr(), capi.DTYPE_U16, frames.shape[0], W * 2, kw, bufs["var"].data_ptr(), bufs["decorr"].data_ptr(),
                                     bufs["cdecorr"].data_ptr(), bufs["power"].data_ptr())
    if ev is not None:
        ss.still_running(ev, "process_angio_device")
        fill_on.synchronize()
    r.synchronize()
    return _collect(bufs, NAMES, 0, (G, H, D))


def test_process_angio_device_behind_a_stall_matches_a_quiet_run_on_a_second_handle():
    W = 200
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    second = _chain_handle(W, True)
    host = angiography.process_angio(second, frames, CHAIN_KW)
    quiet = _process_device(second, frames, W, CHAIN_KW)
    second.close()
    _same(quiet, host, "device memory, the chain form")
    r = _chain_handle(W, True)
    _process_device(r, frames, W, CHAIN_KW)   # the warm call: the run-time compile, every workspace
    S = _busy_stream()
    r.set_stream(S.cuda_stream)
    try:
        busy = _process_device(r, frames, W, CHAIN_KW, fill_on=S)
    finally:
        S.synchronize()
        r.set_stream(None)
    r.close()
    _same(busy, quiet, "the chain form behind a stall")
