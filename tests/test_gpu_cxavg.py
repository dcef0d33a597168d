"""GPU tests of the coherent-averaging stage (include/fdoct_cxavg.h; fdoct_amd/coherent.py), held to tests/cxavg_model.py on the
catalogue of tests/cxavg_cases.py: every case against the truth by the project's adjudication, in both memory spaces on each side
and from an input pointer that is only 8-byte aligned; both kernel forms at their boundary and every instantiation of the register form; a sliding call's groups against calls
on their frames alone; a group's isolation from its neighbours and from its place in the call, beyond one pass of the capped grid;
bit-identity across subsets of outputs and runs; every refusal on poisoned outputs; the chain form; stream order behind a stall."""
import itertools

import numpy as np
import pytest

import cxavg_cases as cc
import cxavg_model as cm
import stream_stall as ss
from fdoct_amd import Config, FdoctError, Reconstructor, capi, coherent, synth

pytestmark = pytest.mark.gpu

NAMES = coherent.WANTS
IDS = [c["what"] for c in cc.CASES]
HOST, DEV = capi.MEM_HOST, capi.MEM_DEVICE
WORDS = {"mean": 2, "mag": 1, "incoh": 1, "coh": 1}    # floats a pixel


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
    return {w: np.full((G, H, D * WORDS[w]), np.nan, np.float32) for w in want}


def _untouched(outs):
    for w, a in outs.items():
        assert np.isnan(a).all(), w + " was written by a refused call"


def _busy_stream():
    """The caller's stream of the stalled runs: a high-priority one, so that torch's default pool keeps its turn (tests/test_gpu_vibro.py)."""
    import torch
    return torch.cuda.Stream(priority=-1)


def _run(rec, X, kw, in_space=HOST, out_space=HOST, want=NAMES, off=0, in_off=0, fill_on=None):
    """fdoct_cxavg on pairs in `in_space` into NaN-filled buffers in `out_space`, every output `off` bytes into its buffer and the
    device input `in_off` pairs into its own; what was asked for comes back, and nothing else was written.  fill_on: the input
    arrives on that stream, behind a stall."""
    import torch
    X = np.ascontiguousarray(X)
    T, H, D = X.shape
    p = coherent.params(**kw)
    G = (T - p.repeats) // p.stride + 1
    n = G * H * D
    keep = []
    if in_space == DEV:
        flat = np.concatenate([np.zeros(2 * in_off, np.float32), X.view(np.float32).reshape(-1)])
        src = torch.from_numpy(flat).cuda()
        d_in = torch.zeros_like(src) if fill_on is not None else src
        keep += [src, d_in]
        in_ptr = d_in.data_ptr() + 8 * in_off
    else:
        assert fill_on is None and in_off == 0
        in_ptr = X.ctypes.data
    if out_space == DEV:
        bufs = {w: torch.full((n * WORDS[w] + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
        base = {w: bufs[w].data_ptr() for w in NAMES}
    else:
        bufs = {w: np.full(n * WORDS[w] + 8, np.nan, np.float32) for w in NAMES}
        base = {w: bufs[w].ctypes.data for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    ptr = lambda w: base[w] + off * WORDS[w] if w in want else None   # noqa: E731
    rec._check(rec.lib.fdoct_cxavg(rec.h, in_ptr, in_space, T, H, D, p, ptr("mean"), ptr("mag"), ptr("incoh"), ptr("coh"), out_space))
    if ev is not None:
        ss.still_running(ev, "cxavg_device")
        fill_on.synchronize()
    rec.synchronize()
    return _collect(bufs, want, off, (G, H, D))


def _collect(bufs, want, off, shape):
    """off: bytes into a float buffer, twice that into the pairs' (which keeps them 8-byte aligned)."""
    out, n = {}, int(np.prod(shape))
    for w in NAMES:
        flat = bufs[w] if isinstance(bufs[w], np.ndarray) else bufs[w].cpu().numpy()
        k, m = off // 4 * WORDS[w], n * WORDS[w]
        if w in want:
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + m:]).all(), w + ": written outside the result"
            v = flat[k:k + m].copy()
            out[w] = (v.view(np.complex64) if w == "mean" else v).reshape(shape)
        else:
            assert np.isnan(flat).all(), w + ": written though not asked for"
    return out


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=IDS)
def test_every_case_against_the_model_in_both_memory_spaces(rec, i):
    c = cc.CASES[i]
    X, refs = cc.case_refs(i)
    kw = cc.case_args(c)
    info = coherent.plan(kw, X.shape[0], c["H"], c["D"])
    groups, form, _, ws = cm.geometry(X.shape[0], c["repeats"], c["stride"], c["H"], c["D"], c["align"])
    assert (info["groups"], info["form"], info["workspace_bytes"]) == (groups, form, ws)
    got = coherent.cxavg(rec, X, kw)
    assert set(got) == set(NAMES) and all(a.shape == (groups, c["H"], c["D"]) for a in got.values())
    cm.check(got, X, c["what"], refs=refs, **kw)
    for ins, outs in ((DEV, DEV), (HOST, DEV), (DEV, HOST)):
        _same(_run(rec, X, kw, ins, outs, off=4 if outs == DEV else 0), got, "memory spaces %d -> %d" % (ins, outs))
    # a device input one pair into its allocation: rows that are only 8-byte aligned whatever the depths
    _same(_run(rec, X, kw, DEV, DEV, in_off=1), got, "the input offset by one pair")


def test_the_catalogue_runs_both_forms_at_their_boundary():
    seen = {}
    for c in cc.CASES:
        info = coherent.plan(cc.case_args(c), c["frames"][0] * c["frames"][1], c["H"], c["D"])
        seen.setdefault(info["form"], set()).add((c["repeats"], c["D"]))
    for N, D in ((8, 512), (2, 2048)):
        assert (N, D) in seen[coherent.FORM_REGISTER] and (N, D + 1) in seen[coherent.FORM_STREAMING]
    # ... and the boundary is where plan says it is, whatever the other arguments
    for N, D in ((2, 2048), (3, 1024), (4, 1024), (5, 512), (8, 512), (9, 256), (16, 256)):
        assert coherent.plan(dict(repeats=N), N, 3, D)["form"] == coherent.FORM_REGISTER
        assert coherent.plan(dict(repeats=N), N, 3, D + 1)["form"] == coherent.FORM_STREAMING
    assert coherent.plan(dict(repeats=17), 17, 3, 1)["form"] == coherent.FORM_STREAMING


@pytest.mark.parametrize("what", ["sliding, N 3, stride 1, 6 frames of 4 x 130, align 1", "sliding, N 4, stride 2, 8 frames of 2 x 1100, align 2 (streaming)"])
def test_a_sliding_calls_groups_are_calls_on_their_frames_alone(rec, what):
    i = cc.index(what)
    c = cc.CASES[i]
    X, _ = cc.case_refs(i)
    kw = cc.case_args(c)
    N, S = c["repeats"], c["stride"]
    got = coherent.cxavg(rec, X, kw)
    G = (X.shape[0] - N) // S + 1
    assert G >= 3 and got["mag"].shape[0] == G
    for g in range(G):
        alone = coherent.cxavg(rec, X[g * S:g * S + N], kw)
        _same({w: got[w][g:g + 1] for w in NAMES}, alone, "group %d" % g)


ISO = dict(repeats=3, ref=1, align=2, align_range=(5, 40))


@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan", "1e30"])
def test_a_group_does_not_read_its_neighbours(rec, fill):
    mid = cc.ac.field(1, 3, 5, 65, 31, kind="vessel", bulk_phase=np.pi)
    alone = coherent.cxavg(rec, mid, ISO)
    X = np.full((9, 5, 65), complex(fill, fill), np.complex64)
    X[3:6] = mid
    got = coherent.cxavg(rec, X, ISO)
    _same({w: got[w][1:2] for w in NAMES}, alone, "the middle group")
    assert not np.isfinite(got["incoh"][0]).any() and not np.isfinite(got["incoh"][2]).any()    # (1e30 squared is no float)


@pytest.mark.parametrize("align", [1, 2])
def test_an_items_place_in_the_call_does_not_change_a_bit(rec, align):
    cus = _cus()
    G = cc.placement_items(cus)
    kw = dict(repeats=2, ref=1, align=align, align_range=(1, 2))
    info = coherent.plan(kw, 2 * G, 1, 3)
    assert info["groups"] == G and cc.ac.beyond(G, cc.resident(cus)), (G, cus)     # one A-scan a group: more than one pass of the capped grid
    X = cc.ac.field(G, 2, 1, 3, 41, kind="independent", bulk_phase=np.pi)
    X[-2:] = X[:2]
    got = coherent.cxavg(rec, X, kw)
    _same({w: got[w][-1] for w in NAMES}, {w: got[w][0] for w in NAMES}, "the group at index 0 and at the last index")
    one = coherent.cxavg(rec, X[:2], kw)
    _same({w: got[w][:1] for w in NAMES}, one, "the group alone")
    cm.check(one, X[:2], "the base call of the placement test, align %d" % align, **kw)
    mid = cc.resident(cus) + 5                                                     # a group of the second pass, bit for bit with its own call
    _same({w: got[w][mid:mid + 1] for w in NAMES}, coherent.cxavg(rec, X[2 * mid:2 * mid + 2], kw), "a group of the second pass")


SUB = dict(repeats=4, ref=2, align=1, align_range=(3, 40))


@pytest.mark.parametrize("shape", [(5, 65), (2, 1100)], ids=["register", "streaming"])
def test_subsets_and_runs_do_not_change_a_bit(rec, shape):
    X = cc.ac.field(2, 4, shape[0], shape[1], 51, kind="vessel", bulk_phase=np.pi)
    for kw in (SUB, dict(SUB, align=2), dict(SUB, align=0)):
        full = coherent.cxavg(rec, X, kw)
        _same(full, coherent.cxavg(rec, X, kw), "a second run")
        for n in (1, 2, 3):
            for want in itertools.combinations(NAMES, n):
                _same(coherent.cxavg(rec, X, kw, want=want), {w: full[w] for w in want}, "subset %s" % (want,))
    dev = _run(rec, X, SUB, DEV, DEV, want=("mag",), off=4)
    _same(dev, {"mag": coherent.cxavg(rec, X, SUB)["mag"]}, "device memory, one output")
    only = coherent.cxavg(rec, X, SUB, want="mean")
    assert only.dtype == np.complex64 and only.shape == (2,) + shape


def test_refusals_leave_poisoned_outputs_alone(rec):
    lib, h = rec.lib, rec.h
    T, H, D = 6, 3, 20
    X = cc.ac.field(2, 3, H, D, 61)
    Xpad = np.zeros(X.size + 1, np.complex64)
    outs = _poisoned(2, H, D)
    good = dict(repeats=3, ref=1, align=1, align_range=(2, 3))

    def call(x=X.ctypes.data, space=HOST, out_space=HOST, T=T, H=H, D=D, p=None, nop=False, **o):
        p = coherent.params(**good) if p is None else p
        ptr = {w: outs[w].ctypes.data for w in NAMES}
        ptr.update(o)
        return lib.fdoct_cxavg(h, x, space, T, H, D, None if nop else p, ptr["mean"], ptr["mag"], ptr["incoh"], ptr["coh"], out_space)

    def P(**kw):
        return coherent.params(**dict(good, **kw))

    # what the stage cannot show without a handle
    assert call(x=Xpad.ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(mean=outs["mean"].ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(coh=outs["mag"].ctypes.data + 8) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(incoh=outs["mean"].ctypes.data + 2 * 2 * H * D * 4 - 4) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(mag=X.ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(T=5) == -1 and call(T=7) == -1 and b"multiple" in lib.fdoct_last_error(h)
    # ... and the rest of the header's list
    assert call(x=None) == -1 and call(nop=True) == -1 and call(space=7) == -1 and call(out_space=-1) == -1
    assert call(p=P(repeats=1)) == -1 and call(p=P(repeats=65)) == -1 and call(T=2) == -1 and call(T=0) == -1 and call(T=65538) == -1
    assert call(p=P(stride=0)) == -1 and call(p=P(stride=4)) == -1 and call(p=P(stride=2)) == -1       # (6 - 3) % 2
    assert call(p=P(ref=-1)) == -1 and call(p=P(ref=3)) == -1
    assert call(p=P(align=3)) == -1 and call(p=P(align=-1)) == -1
    assert call(p=P(align_range=(20, 0))) == -1 and call(p=P(align_range=(19, 2))) == -1 and call(p=P(align=2, align_range=(-1, 0))) == -1
    assert call(H=0) == -1 and call(D=0) == -1 and call(H=1 << 20, D=17) == -1
    assert call(mean=None, mag=None, incoh=None, coh=None) == -1 and b"no output" in lib.fdoct_last_error(h)
    assert call(mag=outs["mag"].ctypes.data + 2) == -1 and call(coh=outs["coh"].ctypes.data + 1) == -1
    _untouched(outs)
    assert np.array_equal(X, cc.ac.field(2, 3, H, D, 61))
    assert call() == 0   # ... and the handle works afterwards
    assert all(np.isfinite(a).all() for a in outs.values())
    with pytest.raises(FdoctError):
        coherent.cxavg(rec, X, good, want=("mag", "mag"))


# ---- end to end: camera frames -> chain -> stage --------------------------------------------------------------------------------
CHAIN_KW = dict(repeats=3, ref=1, align=1, align_range=(40, 80))
H, M, N, D, T = 6, 4, 2560, 320, 6
CHAIN = {"wave, run-time compiled": (200, True, capi.KERNEL_WAVE_JIT), "workgroup per row": (200, False, capi.KERNEL_GENERIC)}


def _chain_handle(W, jit, background=True):
    r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M))
    if background:
        r.set_background(synth.make_background(W).astype(np.float64))
    if not jit:
        r.set_jit(False)
    return r


@pytest.mark.parametrize("name", list(CHAIN), ids=list(CHAIN))
def test_process_cxavg_is_cxavg_of_process_complex(name):
    W, jit, family = CHAIN[name]
    r = _chain_handle(W, jit)
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    X = r.process_complex(frames)
    assert r.last_kernel() == family, r.jit_note()
    assert X.shape == (T, H, D)
    for kw in (CHAIN_KW, dict(repeats=2, stride=1, align=2), dict(repeats=6, align=0)):
        want = coherent.cxavg(r, X, kw)
        got = coherent.process_cxavg(r, frames, kw)
        assert r.last_kernel() == family
        _same(got, want, "the chain form")
        assert all(np.isfinite(a).all() for a in got.values()) and np.count_nonzero(got["mag"]) > 0
    only = coherent.process_cxavg(r, frames, CHAIN_KW, want="mag")
    assert only.dtype == np.float32 and only.shape == (T // 3, H, D)
    assert r.process_complex(frames).tobytes() == X.tobytes()   # the stage changed nothing a later call reads
    # averages = 2 is refused as process_complex refuses it, a frame count off the repeats by the stage; the outputs stay untouched
    outs = _poisoned(2, H, D)
    p = coherent.params(**CHAIN_KW)
    args = (p, outs["mean"].ctypes.data, outs["mag"].ctypes.data, outs["incoh"].ctypes.data, outs["coh"].ctypes.data, HOST)
    assert r.lib.fdoct_process_cxavg(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, 5, 0, *args) == -1
    r.set_averages(2)
    assert r.lib.fdoct_process_cxavg(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, *args) == -2
    assert b"averages" in r.lib.fdoct_last_error(r.h)
    _untouched(outs)
    r.close()


def test_process_cxavg_matches_the_model_on_the_oracles_complex_output():
    """The chain's pairs and the oracle's float composition each lie within complex_model.tolerance of the truth composition, so
    within tx = twice that of each other.  First order in tx, with A = |X| of the oracle's pairs: a modulus moves by tx at most, so
    incoh by mean_n tx_n; C_n moves by sum_b (tx_n A_ref + A_n tx_ref), which turns U_n by that over |C_n|, so S = sum_n U_n X_n
    moves by e_in = sum_n (tx_n + A_n turn_n), mean and mag by e_in / N, coh by (e_in + coh sum_n tx_n) / M.  That is added to the
    stage's own tolerance; nothing of it is taken from the result."""
    import complex_model
    W = 200
    r = _chain_handle(W, True)
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    yb = synth.make_background(W).astype(np.float64)
    Xo = complex_model.model(r.cfg, frames, yb)
    got = coherent.process_cxavg(r, frames, CHAIN_KW)
    r.close()
    kw = CHAIN_KW
    tol = cm.tolerances(Xo, **kw)
    tr = tol["truth"]
    assert tol["condition"] >= cm.CONDITION
    Ng, ref, (first, count) = kw["repeats"], kw["ref"], kw["align_range"]
    A, tx = np.abs(cm.grouped(Xo, Ng).astype(np.complex128)), 2 * cm.grouped(complex_model.tolerance(Xo), Ng)
    s = slice(first, first + count)
    dC = (tx[..., s] * A[:, ref:ref + 1, :, s] + A[..., s] * tx[:, ref:ref + 1, :, s]).sum(-1)
    turn = dC / np.abs(tr["C"])
    turn[:, ref] = 0
    e_in = (tx + A * turn[..., None]).sum(1)
    M = np.where(tr["M"] == 0, 1.0, tr["M"])
    extra = dict(mean=e_in / Ng, mag=e_in / Ng, incoh=tx.sum(1) / Ng, coh=(e_in + tr["coh"] * tx.sum(1)) / M)
    for w in NAMES:
        rat = float((np.abs(got[w] - tr[w]) / (tol[w] + extra[w])).max())
        print("the chain form against the model on the oracle's pairs: %s |gpu - truth| / bound = %.4f" % (w, rat))
        assert rat <= 1.0, w


def test_process_cxavg_without_a_background_is_a_state_error():
    r = _chain_handle(200, True, background=False)
    frames = synth.make_frames(4, T, 200, H, dtype=np.uint16)
    outs = _poisoned(2, H, D)
    p = coherent.params(**CHAIN_KW)
    rc = r.lib.fdoct_process_cxavg(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, p, outs["mean"].ctypes.data, outs["mag"].ctypes.data,
                                   outs["incoh"].ctypes.data, outs["coh"].ctypes.data, HOST)
    assert rc == -5, (rc, r.lib.fdoct_last_error(r.h))
    _untouched(outs)
    r.close()


def _process_device(r, frames, W, kw, fill_on=None):
    import torch
    p = coherent.params(**kw)
    G = (frames.shape[0] - p.repeats) // p.stride + 1
    n = G * H * D
    src = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()
    d_in = torch.zeros_like(src) if fill_on is not None else src
    bufs = {w: torch.full((n * WORDS[w] + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    coherent.process_cxavg_device(r, d_in.data_ptr(), capi.DTYPE_U16, frames.shape[0], W * 2, p, bufs["mean"].data_ptr(), bufs["mag"].data_ptr(),
                                  bufs["incoh"].data_ptr(), bufs["coh"].data_ptr())
    if ev is not None:
        ss.still_running(ev, "process_cxavg_device")
        fill_on.synchronize()
    r.synchronize()
    return _collect(bufs, NAMES, 0, (G, H, D))


def test_the_device_calls_behind_a_stall_match_quiet_runs_on_a_second_handle():
    W = 200
    frames = synth.make_frames(4, T, W, H, dtype=np.uint16)
    X = cc.ac.field(2, 4, 5, 65, 51, kind="vessel", bulk_phase=np.pi)
    kw2 = dict(SUB, align=2)
    second = _chain_handle(W, True)
    quiet = [_run(second, X, SUB, DEV, DEV), _run(second, X, kw2, DEV, DEV), _process_device(second, frames, W, CHAIN_KW)]
    _same(quiet[2], coherent.process_cxavg(second, frames, CHAIN_KW), "device memory, the chain form")
    second.close()
    r = _chain_handle(W, True)
    _run(r, X, SUB, DEV, DEV), _run(r, X, kw2, DEV, DEV), _process_device(r, frames, W, CHAIN_KW)   # the warm calls: the run-time compile, every workspace
    S = _busy_stream()
    r.set_stream(S.cuda_stream)
    try:
        busy = [_run(r, X, SUB, DEV, DEV, fill_on=S), _run(r, X, kw2, DEV, DEV, fill_on=S), _process_device(r, frames, W, CHAIN_KW, fill_on=S)]
    finally:
        S.synchronize()
        r.set_stream(None)
    r.close()
    for b, q, what in zip(busy, quiet, ("cxavg_device, align 1", "cxavg_device, align 2", "process_cxavg_device")):
        _same(b, q, what + " behind a stall")
