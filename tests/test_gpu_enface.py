"""GPU tests of the en-face stage (include/fdoct_enface.h; fdoct_amd/enface.py), held to tests/enface_model.py on the catalogue of
tests/enface_cases.py: every case in both memory spaces on each side -- integer outputs and the maximum bit-equal, the mean bit-equal
to the float32 model and within the derived bound of the float64 truth; pointers off the 16-byte grid; bit-identity across subsets
of outputs, a slab alone or among eight, a position alone or in a batch, and two runs; both kernels beyond one pass of their capped
grid; a NaN A-scan's isolation; every refusal on poisoned outputs; the chain form; stream order behind a stall (the contract of
DESIGN 1, which tests/stream_cases.py does not yet list for this stage)."""
import itertools

import numpy as np
import pytest

import enface_cases as ec
import enface_model as em
import stream_stall as ss
from fdoct_amd import Config, FdoctError, Reconstructor, capi, enface, synth

pytestmark = pytest.mark.gpu

NAMES = enface.WANTS
HOST, DEV = capi.MEM_HOST, capi.MEM_DEVICE
INTS = ("argmax", "surface")
_MODELS = {}


def _case(name):
    """The case and its model, computed once and shared."""
    if name not in _MODELS:
        c = ec.case(name)
        _MODELS[name] = (c, em.model(c["V"], c["p"], c["S"]))
    return _MODELS[name]


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


def _check(got, m, what):
    for w, a in got.items():
        np.testing.assert_array_equal(_bits(a), _bits(m[w]), err_msg="%s: %s against the float32 model" % (what, w))
    if "mean" in got:
        err = np.abs(got["mean"].astype(np.float64) - m["truth"])
        assert np.all(err <= m["bound"]), "%s: mean off the truth by %.3g of its bound" % (what, np.max(err / np.maximum(m["bound"], 1e-300)))


def _wants(kw):
    return NAMES if em.SURFACES[kw.get("surface")] else NAMES[:3]


def _shape(w, ns, P, H):
    return (P, H) if w == "surface" else (ns, P, H)


def _busy_stream():
    """The caller's stream of the stalled runs: a high-priority one, so that torch's default pool keeps its turn (tests/test_gpu_vibro.py)."""
    import torch
    return torch.cuda.Stream(priority=-1)


def _collect(bufs, want, off, shapes):
    """Every buffer is float32 NaN where nothing wrote: the NaN's bits are no depth, so the integer outputs are checked alike."""
    out, k = {}, off // 4
    for w in NAMES:
        flat = bufs[w] if isinstance(bufs[w], np.ndarray) else bufs[w].cpu().numpy()
        if w in want:
            n = int(np.prod(shapes[w]))
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + n:]).all(), w + ": written outside the result"
            a = flat[k:k + n].copy().reshape(shapes[w])
            out[w] = a.view(np.int32) if w in INTS else a
        else:
            assert np.isnan(flat).all(), w + ": written though not asked for"
    return out


def _settle(presync):
    """Before a call: the whole device drained, or (a call made while another waits behind a stall) the default stream alone, which
    holds the buffers' fills and does not wait for the non-blocking stream of the stall."""
    import torch
    if presync:
        torch.cuda.synchronize()
    else:
        torch.cuda.default_stream().synchronize()


def _run(rec, V, kw, S=None, in_space=HOST, out_space=HOST, want=None, off=0, in_off=0, fill_on=None, stall_on=None, then=None, presync=True):
    """fdoct_enface on volumes in `in_space`, `in_off` bytes into their buffers, into NaN-filled buffers in `out_space`, every output
    `off` bytes into its buffer; what was asked for comes back, and nothing else was written.  fill_on: the inputs arrive on that
    stream, behind a stall, and `then` runs right behind the call, before anything is waited for.  stall_on: a stall alone, and the
    outputs (host memory) are read as the call left them."""
    import torch
    V = np.ascontiguousarray(V, np.float32)
    P, H, D = V.shape
    p = enface.params(**kw)
    want = _wants(kw) if want is None else want
    shapes = {w: _shape(w, p.nslabs, P, H) for w in NAMES}
    k, keep, ptrs = in_off // 4, [], []
    for a in (V, S):
        if a is None:
            ptrs.append(None)
            continue
        padded = np.zeros(a.size + 8, np.float32)
        padded[k:k + a.size] = np.ascontiguousarray(a, np.float32).reshape(-1)
        if in_space == DEV:
            src = torch.from_numpy(padded).cuda()
            d_in = torch.zeros_like(src) if fill_on is not None else src
            keep.append((src, d_in))
            ptrs.append(d_in.data_ptr() + in_off)
        else:
            assert fill_on is None
            keep.append(padded)
            ptrs.append(padded.ctypes.data + in_off)
    n = p.nslabs * P * H
    if out_space == DEV:
        bufs = {w: torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
        base = {w: bufs[w].data_ptr() for w in NAMES}
    else:
        bufs = {w: np.full(n + 8, np.nan, np.float32) for w in NAMES}
        base = {w: bufs[w].ctypes.data for w in NAMES}
    _settle(presync)
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            for src, d_in in keep:
                d_in.copy_(src, non_blocking=True)
    if stall_on is not None:
        assert out_space == HOST and fill_on is None
        ss.stall(stall_on)
    ptr = lambda w: base[w] + off if w in want else None   # noqa: E731
    rec._check(rec.lib.fdoct_enface(rec.h, ptrs[0], ptrs[1], in_space, P, H, D, p, ptr("mean"), ptr("max"), ptr("argmax"), ptr("surface"), out_space))
    if stall_on is not None:
        return _collect(bufs, want, off, shapes)
    if ev is not None:
        ss.still_running(ev, "project_into")
    if then is not None:
        then()
    if fill_on is not None:
        fill_on.synchronize()
    rec.synchronize()
    return _collect(bufs, want, off, shapes)


# ---- model parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.NAMES)
def test_every_case_against_the_model_in_both_memory_spaces(rec, name):
    c, m = _case(name)
    V, S, kw = c["V"], c["S"], c["p"]
    P, H, D = V.shape
    info = enface.plan(kw, P, H, D)
    assert info["ascans"] == P * H and info["workspace_bytes"] == (4 * P * H if "surface" in m else 0)
    got = enface.project(rec, V, kw, structure=S)
    assert set(got) == set(_wants(kw)) and all(a.shape == _shape(w, len(kw["slabs"]), P, H) for w, a in got.items())
    _check(got, m, name)
    for ins, outs in ((HOST, HOST), (DEV, DEV), (HOST, DEV), (DEV, HOST)):
        _same(_run(rec, V, kw, S, ins, outs, off=4 if outs == DEV else 0), got, "memory spaces %d -> %d" % (ins, outs))
    one = enface.project(rec, V, kw, want="max", structure=S)
    assert isinstance(one, np.ndarray) and np.array_equal(_bits(one), _bits(got["max"]))


# ---- pointers and ranges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eight slabs", "relative", "structure", "fixed"])
@pytest.mark.parametrize("in_off,off", [(4, 8), (12, 4), (8, 12), (0, 0)])
def test_volumes_and_outputs_off_the_16_byte_grid(rec, name, in_off, off):
    # 257- and 67-depth A-scans start at every residue of 16 bytes already; the offsets move the volume's first byte as well, and
    # at (0, 0) with depths a multiple of 4 (below) every A-scan takes the 16-byte loads
    c, m = _case(name)
    for space in (DEV, HOST):
        _check(_run(rec, c["V"], c["p"], c["S"], space, space, off=off, in_off=in_off), m, "%s at +%d / +%d" % (name, in_off, off))


@pytest.mark.parametrize("D", [64, 256, 260, 1024])
def test_depths_a_multiple_of_four_give_the_same_bits_on_both_load_paths(rec, D):
    V = np.random.default_rng(D).normal(0, 1, (2, 3, D)).astype(np.float32)
    kw = dict(slabs=[(0, D), (1, D - 2), (D // 2, 7), (D - 1, 1)], surface="relative", threshold=0.9, smooth=2, median=3)
    m = em.model(V, kw)
    for in_off in (0, 4):      # 16-byte loads; 4-byte loads of the same depths in the same lanes
        _check(_run(rec, V, kw, None, DEV, DEV, in_off=in_off), m, "depths %d at +%d" % (D, in_off))


RANGES = {
    "overlapping slabs": dict(slabs=[(0, 40), (20, 40), (30, 5), (0, 67)]),
    "a slab of one depth": dict(slabs=[(0, 1), (33, 1), (66, 1)]),
    "smooth 1": dict(slabs=[(0, 8)], surface="absolute", threshold=0.6, smooth=1, median=1),
    "smooth 16": dict(slabs=[(-4, 12)], surface="relative", threshold=0.7, smooth=16, median=3),
    "median 1": dict(slabs=[(0, 8)], surface="relative", threshold=0.8, smooth=3, median=1),
    "median 15 on 3 A-scans": dict(slabs=[(0, 8), (-8, 8)], surface="relative", threshold=0.8, smooth=3, median=15),
    "a search range inside": dict(slabs=[(0, 8)], surface="relative", threshold=0.5, smooth=4, median=3, search=(13, 31)),
}


@pytest.mark.parametrize("name", list(RANGES))
def test_ranges_and_windows(rec, name):
    kw = RANGES[name]
    V = np.random.default_rng(len(name)).uniform(0, 1, (3, 3, 67)).astype(np.float32)
    _check(_run(rec, V, kw, None, DEV, DEV), em.model(V, kw), name)


# ---- bit-identity ------------------------------------------------------------------------------------------------------------------
def test_every_subset_of_outputs_holds_the_same_bits(rec):
    c, m = _case("relative")
    full = _run(rec, c["V"], c["p"], None, DEV, DEV)
    _check(full, m, "all four")
    for k in range(1, 4):
        for want in itertools.combinations(NAMES, k):
            part = _run(rec, c["V"], c["p"], None, DEV, DEV, want=want)
            _same(part, {w: full[w] for w in want}, "the subset %s" % (want,))
    c, m = _case("eight slabs")
    full = _run(rec, c["V"], c["p"], None, DEV, DEV)
    for want in (("mean",), ("max",), ("argmax",), ("mean", "argmax")):
        _same(_run(rec, c["V"], c["p"], None, DEV, DEV, want=want), {w: full[w] for w in want}, "without a surface, %s" % (want,))


@pytest.mark.parametrize("name", ["eight slabs", "relative"])
def test_a_slab_alone_holds_the_bits_it_has_among_others(rec, name):
    c, m = _case(name)
    kw = dict(c["p"])
    if name == "relative":
        kw["slabs"] = kw["slabs"] + [(-40, 30), (5, 1), (0, 257), (200, 57)]
    assert len(kw["slabs"]) == 8
    full = _run(rec, c["V"], kw, None, DEV, DEV)
    for s, slab in enumerate(kw["slabs"]):
        alone = _run(rec, c["V"], dict(kw, slabs=[slab]), None, DEV, DEV)
        _same({w: alone[w][0] for w in NAMES[:3]}, {w: full[w][s] for w in NAMES[:3]}, "slab %d of 8" % s)


def test_a_position_alone_holds_the_bits_it_has_in_a_batch_and_two_runs_agree(rec):
    c, m = _case("clipped")
    V, kw = c["V"], c["p"]
    assert V.shape[0] == 3
    full = _run(rec, V, kw, None, DEV, DEV)
    _same(_run(rec, V, kw, None, DEV, DEV), full, "two runs")
    for pos in (0, 2):
        alone = _run(rec, V[pos:pos + 1], kw, None, DEV, DEV)
        _same({w: alone[w][..., 0, :] for w in alone}, {w: full[w][..., pos, :] for w in full}, "position %d" % pos)


# ---- beyond one pass of the capped grid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface", [None, "relative"], ids=["projection kernel", "both kernels"])
def test_more_a_scans_than_one_pass_of_the_grid(rec, surface):
    H, D = 70, 40
    kw = dict(slabs=[(0, 40), (-3, 9), (5, 1)] if surface else [(0, 40), (3, 9), (5, 1)], surface=surface, threshold=0.6, smooth=3, median=5)
    base = np.random.default_rng(7).uniform(0, 1, (1, H, D)).astype(np.float32)
    want = _run(rec, base, kw, None, DEV, DEV)
    _check(want, em.model(base, kw), "the base batch")
    per_cu = enface.plan(kw, 65536, H, D)["workgroups"] // 256          # the cap of both grids, per compute unit
    assert per_cu == 8
    waves = per_cu * _cus() * 4                                         # A-scans one pass takes
    P = (waves + H - 1) // H + 2
    assert P * H > waves + H and P <= 65536
    got = _run(rec, np.repeat(base, P, axis=0), kw, None, DEV, DEV)
    for w in got:
        exp = np.repeat(want[w], P, axis=-2)
        np.testing.assert_array_equal(_bits(got[w]), _bits(exp), err_msg=w)


# ---- a NaN A-scan -------------------------------------------------------------------------------------------------------------------
def test_a_nan_a_scan_changes_no_other(rec):
    c, m = _case("relative")
    V, kw = c["V"], c["p"]
    S = V.copy()
    clean = _run(rec, V, kw, S, DEV, DEV)
    _check(clean, m, "the clean run")
    # in V only: the surface comes from S, so every other A-scan -- and this one's surface -- keeps its bits
    Vn = V.copy()
    Vn[1, 33, :] = np.nan
    got = _run(rec, Vn, kw, S, DEV, DEV)
    others = np.ones(V.shape[:2], bool)
    others[1, 33] = False
    np.testing.assert_array_equal(got["surface"], clean["surface"])
    for w in NAMES[:3]:
        np.testing.assert_array_equal(_bits(got[w][:, others]), _bits(clean[w][:, others]), err_msg=w)
    # in S only: that A-scan has no crossing and takes its neighbours' surface; where the model's surface is the clean one the bits are
    Sn = S.copy()
    Sn[0, 20, :] = np.nan
    mn = em.model(V, kw, Sn)
    assert mn["z0"][0, 20] == -1 and np.array_equal(np.delete(mn["z0"].reshape(-1), 20), np.delete(m["z0"].reshape(-1), 20))
    got = _run(rec, V, kw, Sn, DEV, DEV)
    _check(got, mn, "a NaN A-scan in the structure volume")
    keep = mn["surface"] == m["surface"]
    assert keep.sum() >= keep.size - 5 and keep[1].all()
    for w in NAMES[:3]:
        np.testing.assert_array_equal(_bits(got[w][:, keep]), _bits(clean[w][:, keep]), err_msg=w)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_alone(rec):
    lib, h = rec.lib, rec.h
    P, H, D = 2, 3, 67
    V = np.random.default_rng(3).uniform(0, 1, (P, H, D)).astype(np.float32)
    Vpad = np.zeros(V.size + 1, np.float32)
    good = dict(slabs=[(0, 30), (-5, 10)], surface="relative", threshold=0.5, smooth=4, median=3)
    outs = {w: np.full(2 * P * H, np.nan, np.float32) for w in NAMES}

    def call(v=V.ctypes.data, s=None, space=HOST, out_space=HOST, P=P, H=H, D=D, p=None, nop=False, **o):
        p = enface.params(**good) if p is None else p
        ptr = {w: outs[w].ctypes.data for w in NAMES}
        ptr.update(o)
        return lib.fdoct_enface(h, v, s, space, P, H, D, None if nop else p, ptr["mean"], ptr["max"], ptr["argmax"], ptr["surface"], out_space)

    def Q(**kw):
        return enface.params(**dict(good, **kw))

    # what the plan cannot show: pointers, memory spaces, overlaps
    assert call(v=None) == -1 and call(nop=True) == -1 and call(space=7) == -1 and call(out_space=-1) == -1
    assert call(v=Vpad.ctypes.data + 2) == -1 and b"4 bytes" in lib.fdoct_last_error(h)
    assert call(s=Vpad.ctypes.data + 1) == -1 and b"4 bytes" in lib.fdoct_last_error(h)
    assert call(mean=outs["mean"].ctypes.data + 2) == -1 and call(surface=outs["surface"].ctypes.data + 1) == -1
    assert call(max=outs["mean"].ctypes.data + 8) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(argmax=V.ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    S = V.copy()
    assert call(s=S.ctypes.data, surface=S.ctypes.data + 64) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(mean=None, max=None, argmax=None, surface=None) == -1 and b"no output" in lib.fdoct_last_error(h)
    fixed = enface.params(slabs=[(0, 30)])
    assert call(p=fixed) == -1 and b"out_surface" in lib.fdoct_last_error(h)
    assert call(p=fixed, surface=None, s=S.ctypes.data) == -1 and b"structure" in lib.fdoct_last_error(h)
    # ... and the rest of the header's list
    assert call(P=0) == -1 and call(P=65537) == -1 and call(H=0) == -1 and call(D=0) == -1 and call(H=1 << 20, D=17) == -1
    ps = Q()
    ps.surface = 3
    assert call(p=ps) == -1 and call(p=Q(smooth=0)) == -1 and call(p=Q(smooth=17)) == -1
    assert call(p=Q(search=(67, 0))) == -1 and call(p=Q(search=(0, 68))) == -1 and call(p=Q(search=(10, 3))) == -1
    assert call(p=Q(threshold=float("nan"))) == -1 and call(p=Q(threshold=0.0)) == -1 and call(p=Q(threshold=1.5)) == -1
    assert call(p=Q(median=2)) == -1 and call(p=Q(median=17)) == -1
    pn = Q()
    pn.nslabs = 9
    assert call(p=pn) == -1 and call(p=Q(slabs=[])) == -1 and call(p=Q(slabs=[(0, 0)])) == -1
    assert call(p=Q(slabs=[(67, 1)])) == -1 and call(p=Q(slabs=[(-67, 80)])) == -1
    assert call(p=enface.params(slabs=[(-1, 5)]), surface=None) == -1 and call(p=enface.params(slabs=[(67, 5)]), surface=None) == -1
    for w, a in outs.items():
        assert np.isnan(a).all(), w + " was written by a refused call"
    assert call() == 0   # ... and the handle works afterwards
    assert not any(np.isnan(a[:P * H]).any() for a in outs.values())
    with pytest.raises(FdoctError):
        enface.project(rec, V, good, want=("mean", "mean"))
    with pytest.raises(FdoctError):
        enface.project(rec, V, dict(slabs=[(0, 5)]), want="surface")


# ---- end to end: camera frames -> chain -> stage ------------------------------------------------------------------------------------
CW, CH, CN, CD = 64, 4, 128, 128
CHAIN_KW = dict(slabs=[(0, 128), (-6, 12), (20, 30)], surface="relative", threshold=0.5, smooth=4, median=3)


def _chain_handle(averages=1, background=True):
    r = Reconstructor(Config(width=CW, height=CH, numfftpoints=CN, numdisplaypoints=CD, averages=averages))
    if background:
        r.set_background(synth.make_background(CW).astype(np.float64))
    return r


@pytest.mark.parametrize("averages", [1, 2])
def test_process_project_is_the_model_of_process(averages):
    r = _chain_handle(averages)
    T = 6
    frames = synth.make_frames(4, T, CW, CH, dtype=np.uint16)
    bscan, db = r.process(frames)
    family = r.last_kernel()
    assert bscan.shape == db.shape == (T // averages, CH, CD) and family != capi.KERNEL_NONE
    for source, vol in (("linear", bscan), ("db", db)):
        for kw in (CHAIN_KW, dict(slabs=[(5, 100), (127, 1)])):
            got = enface.process_project(r, frames, kw, source=source)
            assert r.last_kernel() == family
            _check(got, em.model(vol, kw), "the chain form, %s" % source)
            _same(got, enface.project(r, vol, kw), "the chain form against the stage on process()'s volume")
    only = enface.process_project(r, frames, CHAIN_KW, want="surface")
    assert only.dtype == np.int32 and only.shape == (T // averages, CH)
    again = r.process(frames)
    assert again[0].tobytes() == bscan.tobytes() and again[1].tobytes() == db.tobytes()   # the stage changed nothing a later call reads
    r.close()


def test_process_project_refusals_are_the_chains():
    T = 6
    frames = synth.make_frames(4, T, CW, CH, dtype=np.uint16)
    p = enface.params(**CHAIN_KW)
    outs = {w: np.full(3 * T * CH, np.nan, np.float32) for w in NAMES}
    args = (p, outs["mean"].ctypes.data, outs["max"].ctypes.data, outs["argmax"].ctypes.data, outs["surface"].ctypes.data, HOST)
    r = _chain_handle(1, background=False)
    rc = r.lib.fdoct_process_enface(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, 1, *args)
    assert rc == -5, (rc, r.lib.fdoct_last_error(r.h))
    r.close()
    r = _chain_handle(1)
    lib, h = r.lib, r.h
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, 2, *args) == -1 and b"source" in lib.fdoct_last_error(h)
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, -1, *args) == -1
    assert lib.fdoct_process_enface(h, None, capi.DTYPE_U16, HOST, T, 0, 1, *args) == -1
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, 0, 0, 1, *args) == -1
    assert lib.fdoct_process_enface(h, frames.ctypes.data, 9, HOST, T, 0, 1, *args) == -1
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 2, 1, *args) == -1 and b"pitch" in lib.fdoct_last_error(h)
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, 5, T, 0, 1, *args) == -1
    bad = enface.params(**dict(CHAIN_KW, slabs=[(128, 1)]))
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, 1, bad, *args[1:]) == -1
    r.set_raw_magnitudes(True)
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, 1, *args) == -1 and b"raw magnitudes" in lib.fdoct_last_error(h)
    r.set_raw_magnitudes(False)
    r.set_averages(4)
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, 1, *args) == -1 and b"averages" in lib.fdoct_last_error(h)
    r.set_averages(1)
    for w, a in outs.items():
        assert np.isnan(a).all(), w + " was written by a refused call"
    assert lib.fdoct_process_enface(h, frames.ctypes.data, capi.DTYPE_U16, HOST, T, 0, 1, *args) == 0
    r.close()


# ---- stream order -------------------------------------------------------------------------------------------------------------------
SO_KW = dict(slabs=[(0, 64), (-10, 20), (64, 64)], surface="relative", threshold=0.5, smooth=4, median=5)


def _quiet_handle():
    return Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))


def test_project_into_behind_a_stall_matches_a_quiet_run_on_a_second_handle(rec):
    c, m = _case("relative")
    second = _quiet_handle()
    quiet = _run(second, c["V"], SO_KW, c["V"] + 0, DEV, DEV)
    second.close()
    _check(quiet, em.model(c["V"], SO_KW), "the quiet run")
    _run(rec, c["V"], SO_KW, c["V"] + 0, DEV, DEV)   # the warm call: every workspace has its size
    S = _busy_stream()
    rec.set_stream(S.cuda_stream)
    try:
        busy = _run(rec, c["V"], SO_KW, c["V"] + 0, DEV, DEV, fill_on=S)
    finally:
        S.synchronize()
        rec.set_stream(None)
    _same(busy, quiet, "behind a stall")


def _process_into(r, frames, kw, source="db", fill_on=None, then=None, presync=True):
    """process_project_into on device-resident frames; `then` runs right behind the call, before anything is waited for."""
    import torch
    p = enface.params(**kw)
    G = frames.shape[0] // r.cfg.averages
    shapes = {w: _shape(w, p.nslabs, G, CH) for w in NAMES}
    src = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()
    d_in = torch.zeros_like(src) if fill_on is not None else src
    bufs = {w: torch.full((p.nslabs * G * CH + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    _settle(presync)
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    enface.process_project_into(r, d_in.data_ptr(), capi.DTYPE_U16, frames.shape[0], CW * 2, source, kw, bufs["mean"].data_ptr(), bufs["max"].data_ptr(),
                                bufs["argmax"].data_ptr(), bufs["surface"].data_ptr())
    if ev is not None:
        ss.still_running(ev, "process_project_into")
    if then is not None:
        then()
    if fill_on is not None:
        fill_on.synchronize()
    r.synchronize()
    return _collect(bufs, NAMES, 0, shapes)


def test_process_project_into_behind_a_stall_matches_a_quiet_run_on_a_second_handle():
    frames = synth.make_frames(4, 6, CW, CH, dtype=np.uint16)
    second = _chain_handle()
    host = enface.process_project(second, frames, CHAIN_KW)
    quiet = _process_into(second, frames, CHAIN_KW)
    second.close()
    _same(quiet, host, "device memory, the chain form")
    r = _chain_handle()
    _process_into(r, frames, CHAIN_KW)   # the warm call: the route's tables, every workspace
    S = _busy_stream()
    r.set_stream(S.cuda_stream)
    try:
        busy = _process_into(r, frames, CHAIN_KW, fill_on=S)
    finally:
        S.synchronize()
        r.set_stream(None)
    r.close()
    _same(busy, quiet, "the chain form behind a stall")


def test_a_call_that_outgrows_the_workspaces_leaves_the_queued_call_intact():
    # call A (2 frames) is queued behind a stall; call B (6 frames) needs a larger ws_enf_vol and ws_enf_surf and is made while A waits
    frames = synth.make_frames(4, 6, CW, CH, dtype=np.uint16)
    second = _chain_handle()
    quiet_a, quiet_b = _process_into(second, frames[:2], CHAIN_KW), _process_into(second, frames, CHAIN_KW)
    second.close()
    r = _chain_handle()
    _process_into(r, frames[:2], CHAIN_KW)   # the warm call: the workspaces have call A's size
    S = _busy_stream()
    r.set_stream(S.cuda_stream)
    later = {}
    try:
        busy_a = _process_into(r, frames[:2], CHAIN_KW, fill_on=S, then=lambda: later.update(b=_process_into(r, frames, CHAIN_KW, presync=False)))
    finally:
        S.synchronize()
        r.set_stream(None)
    r.close()
    _same(busy_a, quiet_a, "call A, queued when the workspaces grew")
    _same(later["b"], quiet_b, "call B, the larger one")


def test_a_stage_call_that_outgrows_the_surfaces_leaves_the_queued_call_intact():
    c, m = _case("relative")
    V = c["V"]
    second = _quiet_handle()
    quiet_a, quiet_b = _run(second, V[:1], SO_KW, None, DEV, DEV), _run(second, V, SO_KW, None, DEV, DEV)
    second.close()
    r = _quiet_handle()
    _run(r, V[:1], SO_KW, None, DEV, DEV)    # the warm call: ws_enf_surf has call A's size
    S = _busy_stream()
    r.set_stream(S.cuda_stream)
    later = {}
    try:
        busy_a = _run(r, V[:1], SO_KW, None, DEV, DEV, fill_on=S, then=lambda: later.update(b=_run(r, V, SO_KW, None, DEV, DEV, presync=False)))
    finally:
        S.synchronize()
        r.set_stream(None)
    r.close()
    _same(busy_a, quiet_a, "call A, queued when the surfaces' workspace grew")
    _same(later["b"], quiet_b, "call B, the larger one")


def test_host_memory_outputs_return_drained(rec):
    c, m = _case("relative")
    quiet = _run(rec, c["V"], SO_KW, None, DEV, HOST)
    S = _busy_stream()
    rec.set_stream(S.cuda_stream)
    try:
        got = _run(rec, c["V"], SO_KW, None, DEV, HOST, stall_on=S)   # read as the call left them
    finally:
        S.synchronize()
        rec.set_stream(None)
    _same(got, quiet, "host outputs behind a stall")
