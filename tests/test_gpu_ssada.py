"""GPU tests of the split-spectrum stage (include/fdoct_ssada.h; fdoct_amd/ssada.py), held to tests/ssada_model.py on the catalogue
of tests/ssada_cases.py: the band A-scans of every case against the truth by the project's adjudication, in host and in device
memory; the identity; the window stage bit for bit against angiography.angio_device on the call's own bands; the band means bit
for bit against numpy; subsets, runs, passes of the workspace and a group's isolation; the capped grids beyond one pass; the chain
form; every refusal on poisoned outputs; one sanity case of the physics.

The worst ratios of every case are printed before anything is asserted (profiles/ssada_ratios.txt is that output from one run)."""
import itertools

import numpy as np
import pytest

import angio_cases as ac
import ssada_cases as sc
import ssada_model as sm
from fdoct_amd import Config, FdoctError, Reconstructor, angiography, capi, ssada, synth

pytestmark = pytest.mark.gpu

NAMES = ssada.WANTS
IDS = [c["what"] for c in sc.CASES]
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
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def _same(a, b, what=""):
    assert set(a) == set(b), (what, set(a), set(b))
    for w in a:
        np.testing.assert_array_equal(_bits(a[w]), _bits(b[w]), err_msg="%s: %s" % (what, w))


def _shapes(G, M, R, H, dc):
    return {"decorr": (G, H, dc), "power": (G, H, dc), "band_decorr": (G, M, H, dc), "bands": (G, M, R, H, dc, 2)}


def _params(kw, n):
    return kw if isinstance(kw, ssada._CParams) else ssada.params(n=n, **kw)


def _run(rec, X, kw, in_space=HOST, out_space=HOST, want=NAMES, off=0):
    """fdoct_ssada on pairs in `in_space` into NaN-filled buffers in `out_space`, every output `off` bytes into its buffer (a
    multiple of 8); what was asked for comes back -- bands as complex64 -- and nothing else was written."""
    import torch
    X = np.ascontiguousarray(X)
    T, H, n = X.shape
    p = _params(kw, n)
    info = ssada.plan(p, T, H, n)
    shapes = _shapes(info["groups"], p.bands, p.repeats, H, info["depth_count"])
    keep = []
    if in_space == DEV:
        src = torch.from_numpy(X.view(np.float32).reshape(-1).copy()).cuda()
        keep.append(src)
        in_ptr = src.data_ptr()
    else:
        in_ptr = X.ctypes.data
    if out_space == DEV:
        bufs = {w: torch.full((int(np.prod(shapes[w])) + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
        base = {w: bufs[w].data_ptr() for w in NAMES}
    else:
        bufs = {w: np.full(int(np.prod(shapes[w])) + 8, np.nan, np.float32) for w in NAMES}
        base = {w: bufs[w].ctypes.data for w in NAMES}
    torch.cuda.synchronize()
    ptr = lambda w: base[w] + off if w in want else None   # noqa: E731
    rec._check(rec.lib.fdoct_ssada(rec.h, in_ptr, in_space, T, H, n, p, ptr("decorr"), ptr("band_decorr"), ptr("power"), ptr("bands"), out_space))
    rec.synchronize()
    return _collect(bufs, want, off, shapes)


def _collect(bufs, want, off, shapes):
    out, k = {}, off // 4
    for w in NAMES:
        flat = bufs[w] if isinstance(bufs[w], np.ndarray) else bufs[w].cpu().numpy()
        n = int(np.prod(shapes[w]))
        if w in want:
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + n:]).all(), w + ": written outside the result"
            a = flat[k:k + n].copy().reshape(shapes[w])
            out[w] = a.view(np.complex64)[..., 0] if w == "bands" else a
        else:
            assert np.isnan(flat).all(), w + ": written though not asked for"
    return out


# ---- 1. the band A-scans against the truth -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_every_cases_bands_against_the_truth_in_both_memory_spaces(rec, i):
    c = sc.CASES[i]
    X, f, t = sc.case_refs(i)
    kw = sc.case_args(c)
    got = ssada.ssada(rec, X, kw)
    assert set(got) == set(NAMES) and got["bands"].shape == t["bands"].shape and got["bands"].dtype == np.complex64
    sm.check_bands(got["bands"], t, f, c["N"], c["what"] + " (host memory)")
    dev = _run(rec, X, kw, DEV, DEV, off=8)
    sm.check_bands(dev["bands"], t, f, c["N"], c["what"] + " (device memory)")
    _same(dev, got, "device memory against host memory")
    for ins, outs in ((HOST, DEV), (DEV, HOST)):
        _same(_run(rec, X, kw, ins, outs), got, "memory spaces %d -> %d" % (ins, outs))
    for (fr, r) in sc.zero_rows(c):                      # a row of zeros: tolerance 0
        g, n = divmod(fr, c["repeats"])
        assert not got["bands"][g, :, n, r].any()
    assert all(np.isfinite(got[w]).all() for w in NAMES)


# ---- 2. the identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,depth", [(16, (0, 16)), (60, (7, 11)), (1000, (0, 0)), (4096, (65, 129))], ids=["N 16", "N 60", "N 1000", "N 4096"])
def test_one_band_of_ones_gives_the_ascans_back(rec, N, depth):
    X = ac.field(1, 2, 3, N, 21, kind="independent")
    kw = dict(repeats=2, bands=1, sigma=1e12, depth=depth)
    assert (ssada.band_table(kw, N) == np.float32(1)).all()
    got = ssada.ssada(rec, X, kw, want="bands")
    _, _, _, d0, dc = sm.resolve(N, 1, 1e12, (0, 0), depth)
    want = X.reshape(1, 2, 3, N)[:, None, :, :, d0:d0 + dc].astype(np.complex128)
    norm = np.sqrt((np.abs(X.astype(np.complex128)) ** 2).sum(-1)).reshape(1, 1, 2, 3)
    t = dict(bands=want, norm=norm)
    row, bins = sm.band_ratios(got, t, N)
    print("identity, N %d: |gpu - X| / tol: row %.4g, bin %.4g" % (N, row, bins))
    assert row <= 0.5 and bins <= 0.5


# ---- 3. the window stage is fdoct_angio's, bit for bit -----------------------------------------------------------------------------
def _angio_of_bands(rec, bands, win):
    """angiography.angio_device on every (group, band) slice of out_bands: (decorr, power), each (G, M, H, dc)."""
    import torch
    G, M, R, H, dc = bands.shape
    d_b = torch.from_numpy(np.ascontiguousarray(bands).view(np.float32).reshape(-1).copy()).cuda()
    d_dec = torch.full((G * M * H * dc,), float("nan"), dtype=torch.float32, device="cuda")
    d_pow = torch.full((G * M * H * dc,), float("nan"), dtype=torch.float32, device="cuda")
    p = angiography.params(repeats=R, win=win)
    for s in range(G * M):
        angiography.angio_device(rec, d_b.data_ptr() + s * R * H * dc * 8, R, H, dc, p, None, d_dec.data_ptr() + s * H * dc * 4, None,
                                 d_pow.data_ptr() + s * H * dc * 4)
    rec.synchronize()
    return d_dec.cpu().numpy().reshape(G, M, H, dc), d_pow.cpu().numpy().reshape(G, M, H, dc)


WINDOW_CASES = ["N 60, 3 bands, 2 groups of 17, R 3, depths 7..17, window 3 x 5", "N 60, 4 bands, 2 x 5 image, window 16 x 16",
                "N 1024, 4 bands, 2 groups of 4, R 2, depths 65..193, a frame of zeros", "N 4096, 3 bands, 2 A-scans, R 2, window 1 x 1"]


@pytest.mark.parametrize("what", WINDOW_CASES)
def test_band_decorr_and_power_are_angio_of_the_calls_own_bands(rec, what):
    c = sc.CASES[sc.index(what)]
    X = sc.case_field(c)
    kw = dict(sc.case_args(c), min_power=0.0)
    got = _run(rec, X, kw, DEV, DEV)
    dec, pw = _angio_of_bands(rec, got["bands"], c["win"])
    np.testing.assert_array_equal(_bits(got["band_decorr"]), _bits(dec))
    # the per-band power shows through out_power with one band: a sum of one term from 0.f and a division by 1.f change no bit
    one = dict(kw, bands=1, sigma=c["sigma"] if c["sigma"] else 0.5 * sm.resolve(c["N"], c["bands"], None, c["support"])[1] / c["bands"])
    got1 = _run(rec, X, one, DEV, DEV)
    dec1, pw1 = _angio_of_bands(rec, got1["bands"], c["win"])
    np.testing.assert_array_equal(_bits(got1["power"]), _bits(pw1[:, 0]))
    np.testing.assert_array_equal(_bits(got1["decorr"]), _bits(dec1[:, 0]))
    np.testing.assert_array_equal(_bits(got1["band_decorr"]), _bits(dec1))
    # ... and with all bands out_power is the float mean of the per-band powers
    np.testing.assert_array_equal(_bits(got["power"]), _bits(sm.band_mean(pw)))


# ---- 4. the band means, and the mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", [1, 3, 4, 16])
def test_decorr_and_power_are_the_float_band_means_with_the_mask(rec, bands):
    X = ac.field(2, 3, 9, 256, 31, kind="vessel")
    kw = dict(repeats=3, bands=bands, depth=(5, 77), win=(3, 5))
    free = _run(rec, X, kw, DEV, DEV)
    _, pw = _angio_of_bands(rec, free["bands"], (3, 5))
    power = sm.band_mean(pw)
    np.testing.assert_array_equal(_bits(free["power"]), _bits(power))
    np.testing.assert_array_equal(_bits(free["decorr"]), _bits(sm.band_mean(free["band_decorr"])))
    min_power = float(np.float32(np.median(power)))
    got = ssada.ssada(rec, X, dict(kw, min_power=min_power))
    dec, pw2 = sm.band_mean(got["band_decorr"], min_power, pw)
    masked = power < np.float32(min_power)
    assert 0.25 < masked.mean() < 0.75                        # the threshold splits the image
    np.testing.assert_array_equal(_bits(got["decorr"]), _bits(dec))
    np.testing.assert_array_equal(_bits(got["power"]), _bits(power))
    _same({w: got[w] for w in ("band_decorr", "bands", "power")}, {w: free[w] for w in ("band_decorr", "bands", "power")}, "the mask touches out_decorr alone")
    assert not got["decorr"][masked].any() and np.array_equal(_bits(got["decorr"][~masked]), _bits(free["decorr"][~masked]))


# ---- 5. subsets and runs ---------------------------------------------------------------------------------------------------------
SUB0 = dict(repeats=4, bands=3, support=(10, 200), depth=(3, 131), win=(5, 5))


def _median_power(rec, X, kw):
    """A min_power that splits the image: the median of the call's own out_power."""
    return float(np.float32(np.median(ssada.ssada(rec, X, dict(kw, min_power=0.0), want="power"))))


def test_subsets_and_runs_do_not_change_a_bit(rec):
    X = ac.field(2, 4, 5, 240, 51, kind="vessel")
    SUB = dict(SUB0, min_power=_median_power(rec, X, SUB0))
    full = ssada.ssada(rec, X, SUB)
    _same(full, ssada.ssada(rec, X, SUB), "a second run")
    assert np.count_nonzero(full["decorr"]) > 0 and np.count_nonzero(full["decorr"] == 0) > 0      # the mask takes part
    for n in (1, 2, 3):
        for want in itertools.combinations(NAMES, n):
            _same(ssada.ssada(rec, X, SUB, want=want), {w: full[w] for w in want}, "subset %s" % (want,))
            _same(_run(rec, X, SUB, DEV, DEV, want=want, off=8), {w: full[w] for w in want}, "subset %s, device memory" % (want,))
    only = ssada.ssada(rec, X, SUB, want="decorr")
    assert only.dtype == np.float32 and np.array_equal(_bits(only), _bits(full["decorr"]))
    kw = dict(SUB, min_power=0.0)
    full = ssada.ssada(rec, X, kw)
    for w in NAMES:
        _same(ssada.ssada(rec, X, kw, want=(w,)), {w: full[w]}, "alone, no mask")


# ---- 6. passes of the workspace -----------------------------------------------------------------------------------------------------
def test_three_passes_give_the_bits_of_one(rec):
    G, R, H, N, M = 7, 2, 5, 60, 3
    X = ac.field(G, R, H, N, 61, kind="vessel")
    kw = dict(repeats=R, bands=M, depth=(2, 21), win=(3, 5))
    kw["min_power"] = _median_power(rec, X, kw)
    share = sc.group_share(R, M, H, 21)
    one = ssada.ssada(rec, X, kw)
    assert ssada.plan(kw, G * R, H, N)["passes"] == 1
    for cap, passes in ((3 * share + share // 2, 3), (share, 7)):       # 3 + 3 + 1 groups; one group a pass
        capped = dict(kw, max_workspace_bytes=cap)
        assert ssada.plan(capped, G * R, H, N)["passes"] == passes
        _same(ssada.ssada(rec, X, capped), one, "%d passes, host memory" % passes)
        _same(_run(rec, X, capped, DEV, DEV, want=("decorr", "band_decorr", "power")), {w: one[w] for w in ("decorr", "band_decorr", "power")},
              "%d passes, device memory without out_bands" % passes)
        _same(_run(rec, X, capped, DEV, DEV), one, "device memory with out_bands: one pass whatever the cap")
        _same(_run(rec, X, capped, DEV, HOST, want=("bands", "decorr")), {w: one[w] for w in ("bands", "decorr")}, "%d passes, out_bands copied down" % passes)
    out = np.full(G * H * 21, np.nan, np.float32)
    p = ssada.params(n=N, **dict(kw, max_workspace_bytes=share - 1))
    assert rec.lib.fdoct_ssada(rec.h, X.ctypes.data, HOST, G * R, H, N, p, out.ctypes.data, None, None, None, HOST) == -1
    assert b"max_workspace_bytes" in rec.lib.fdoct_last_error(rec.h) and np.isnan(out).all()


# ---- 7. a group's isolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan", "1e30"])
def test_a_group_equals_the_call_on_its_frames_alone(rec, fill):
    kw = dict(repeats=3, bands=4, depth=(0, 60), win=(3, 5))
    mid = ac.field(1, 3, 7, 60, 71, kind="vessel")
    kw["min_power"] = _median_power(rec, mid, kw)
    alone = ssada.ssada(rec, mid, kw)
    X = np.full((9, 7, 60), complex(fill, fill), np.complex64)
    X[3:6] = mid
    got = ssada.ssada(rec, X, kw)
    _same({w: got[w][1:2] for w in NAMES}, alone, "the middle group")
    assert not np.isfinite(got["power"][0]).any() and not np.isfinite(got["power"][2]).any()
    three = ac.field(3, 3, 7, 60, 72, kind="independent")
    all3 = ssada.ssada(rec, three, kw)
    for g in range(3):
        _same({w: all3[w][g:g + 1] for w in NAMES}, ssada.ssada(rec, three[3 * g:3 * g + 3], kw), "group %d alone" % g)


def test_the_capped_grids_beyond_one_pass(rec):
    """One group of 2 repeats of H A-scans of 16 points, 8 depths kept: the split kernel's items and the mean kernel's pixels both
    run more than one and a half passes of their capped grids, the last partial (tests/ssada_cases.py: grid_ascans)."""
    cus = _cus()
    N, dc = 16, 8
    H = sc.grid_ascans(cus, dc)
    assert sc.beyond(2 * H, sc.resident(cus)) and sc.beyond(H * dc, sc.resident(cus) * sc.BLOCK), (H, cus)
    kw = dict(repeats=2, bands=1, sigma=3.0)
    assert ssada.plan(kw, 2, H, N)["workgroups"] == min(2 * H, sc.resident(sc.PLAN_CUS))
    X = ac.field(1, 2, H, N, 81, kind="independent")
    X[:, -1] = X[:, 0]                                               # the last A-scan: the last pass's; the first: the first pass's
    got = ssada.ssada(rec, X, kw)
    t, f = sm.model(X, truth=True, **kw), sm.model(X, **kw)
    sm.check_bands(got["bands"], t, f, N, "beyond one pass of the capped grids, %d A-scans" % H)
    np.testing.assert_array_equal(_bits(got["bands"][..., -1, :]), _bits(got["bands"][..., 0, :]))
    for w in ("decorr", "power", "band_decorr"):                      # 1 x 1 window: a pixel reads its own A-scan only
        np.testing.assert_array_equal(_bits(got[w][..., -1, :]), _bits(got[w][..., 0, :]), err_msg=w)
    np.testing.assert_array_equal(_bits(got["decorr"]), _bits(got["band_decorr"][:, 0]))
    few = ssada.ssada(rec, X[:, :5], kw)
    _same({w: got[w][..., :5, :] for w in NAMES}, few, "the first A-scans alone")
    dec, pw = _angio_of_bands(rec, got["bands"], (1, 1))               # every pixel of every pass: the window stage's own bits
    np.testing.assert_array_equal(_bits(got["band_decorr"]), _bits(dec))
    np.testing.assert_array_equal(_bits(got["power"]), _bits(pw[:, 0]))


# ---- 8. end to end: camera frames -> chain -> stage -----------------------------------------------------------------------------------
CH_H, CH_W, CH_N, CH_T, CH_DC = 4, 64, 128, 6, 41
CHAIN_KW = dict(repeats=3, bands=4, support=(4, 100), depth=(3, CH_DC), win=(3, 5))


def _chain_handle(D=CH_N, background=True):
    r = Reconstructor(Config(width=CH_W, height=CH_H, numfftpoints=CH_N, numdisplaypoints=D))
    if background:
        r.set_background(synth.make_background(CH_W).astype(np.float64))
    return r


def test_process_ssada_is_ssada_of_process_complex():
    r = _chain_handle()
    frames = synth.make_frames(4, CH_T, CH_W, CH_H, dtype=np.uint16)
    X = r.process_complex(frames)
    family = r.last_kernel()
    assert X.shape == (CH_T, CH_H, CH_N)
    probe = ssada.ssada(r, X, CHAIN_KW, want="power")
    for kw in (dict(CHAIN_KW, min_power=float(np.float32(np.median(probe)))), dict(repeats=2, bands=1)):
        want = ssada.ssada(r, X, kw)
        got = ssada.process_ssada(r, frames, kw)
        assert r.last_kernel() == family
        _same(got, want, "the chain form")
        assert all(np.isfinite(a).all() for a in got.values()) and np.count_nonzero(got["decorr"]) > 0
    only = ssada.process_ssada(r, frames, CHAIN_KW, want="decorr")
    assert only.dtype == np.float32 and only.shape == (CH_T // 3, CH_H, CH_DC)
    assert r.process_complex(frames).tobytes() == X.tobytes()   # the stage changed nothing a later call reads
    # device memory on both sides
    import torch
    src = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()
    d_dec = torch.full((2 * CH_H * CH_DC,), float("nan"), dtype=torch.float32, device="cuda")
    ssada.process_ssada_device(r, src.data_ptr(), capi.DTYPE_U16, CH_T, CH_W * 2, CHAIN_KW, d_dec.data_ptr(), None, None, None)
    r.synchronize()
    np.testing.assert_array_equal(_bits(d_dec.cpu().numpy().reshape(2, CH_H, CH_DC)), _bits(only))
    # a frame count off the repeats is refused by the stage, averages = 2 as process_complex refuses it; the outputs stay untouched
    out = np.full(2 * CH_H * CH_DC, np.nan, np.float32)
    p = ssada.params(n=CH_N, **CHAIN_KW)
    assert r.lib.fdoct_process_ssada(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, 5, 0, p, out.ctypes.data, None, None, None, HOST) == -1
    r.set_averages(2)
    assert r.lib.fdoct_process_ssada(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, CH_T, 0, p, out.ctypes.data, None, None, None, HOST) == -2
    assert b"averages" in r.lib.fdoct_last_error(r.h)
    assert np.isnan(out).all()
    r.close()


def test_process_ssada_needs_the_full_length_and_a_background():
    frames = synth.make_frames(4, CH_T, CH_W, CH_H, dtype=np.uint16)
    out = np.full(2 * CH_H * CH_DC, np.nan, np.float32)
    p = ssada.params(n=CH_N, **CHAIN_KW)
    r = _chain_handle(D=CH_N // 2)
    rc = r.lib.fdoct_process_ssada(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, CH_T, 0, p, out.ctypes.data, None, None, None, HOST)
    assert rc == -2 and b"numfftpoints" in r.lib.fdoct_last_error(r.h), (rc, r.lib.fdoct_last_error(r.h))
    with pytest.raises(FdoctError) as e:
        ssada.process_ssada(r, frames, CHAIN_KW)
    assert e.value.code == -2
    r.close()
    r = _chain_handle(background=False)
    rc = r.lib.fdoct_process_ssada(r.h, frames.ctypes.data, capi.DTYPE_U16, HOST, CH_T, 0, p, out.ctypes.data, None, None, None, HOST)
    assert rc == -5, (rc, r.lib.fdoct_last_error(r.h))
    assert np.isnan(out).all()
    r.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_alone(rec):
    lib, h = rec.lib, rec.h
    T, H, N = 6, 3, 60
    good = dict(repeats=3, bands=4, sigma=5.0, support=(4, 40), depth=(2, 20), win=(3, 5))
    X = ac.field(2, 3, H, N, 91)
    Xpad = np.zeros(X.size + 1, np.complex64)
    shapes = _shapes(2, 4, 3, H, 20)
    outs = {w: np.full(int(np.prod(shapes[w])) + 2, np.nan, np.float32) for w in NAMES}

    def call(x=X.ctypes.data, space=HOST, out_space=HOST, T=T, H=H, N=N, p=None, nop=False, **o):
        p = ssada.params(**good) if p is None else p
        ptr = {w: outs[w].ctypes.data for w in NAMES}
        ptr.update(o)
        return lib.fdoct_ssada(h, x, space, T, H, N, None if nop else p, ptr["decorr"], ptr["band_decorr"], ptr["power"], ptr["bands"], out_space)

    def P(**kw):
        return ssada.params(**dict(good, **kw))

    # what the stage cannot show without a handle
    assert call(x=Xpad.ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(power=outs["decorr"].ctypes.data + 8) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(decorr=X.ctypes.data + 16) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(bands=outs["band_decorr"].ctypes.data + 64) == -1 and b"overlap" in lib.fdoct_last_error(h)
    assert call(bands=outs["bands"].ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    assert call(decorr=outs["decorr"].ctypes.data + 2) == -1 and call(band_decorr=outs["band_decorr"].ctypes.data + 1) == -1
    assert call(decorr=None, band_decorr=None, power=None, bands=None) == -1 and b"no output" in lib.fdoct_last_error(h)
    assert call(x=None) == -1 and call(nop=True) == -1 and call(space=7) == -1 and call(out_space=-1) == -1
    # ... and the plan's list, through the call
    assert call(T=5) == -1 and call(T=7) == -1 and b"multiple" in lib.fdoct_last_error(h)
    assert call(N=56) == -2 and call(N=8192) == -2 and call(N=0) == -1
    assert call(p=P(repeats=1)) == -1 and call(p=P(repeats=65)) == -1 and call(p=P(bands=0)) == -1 and call(p=P(bands=17)) == -1
    assert call(T=0) == -1 and call(H=0) == -1 and call(H=1 << 20, p=P(depth=(0, 17))) == -1
    assert call(p=P(support=(60, 0))) == -1 and call(p=P(support=(59, 2))) == -1 and call(p=P(depth=(30, 0))) == -1 and call(p=P(depth=(58, 3))) == -1
    assert call(p=P(sigma=0.0)) == -1 and call(p=P(sigma=float("nan"))) == -1
    assert call(p=P(win=(0, 1))) == -1 and call(p=P(win=(1, 17))) == -1
    assert call(p=P(min_power=float("nan"))) == -1 and call(p=P(min_power=-1.0)) == -1
    assert call(p=P(max_workspace_bytes=100)) == -1
    for w, a in outs.items():
        assert np.isnan(a).all(), w + " was written by a refused call"
    assert np.array_equal(X, ac.field(2, 3, H, N, 91))
    # device memory: the same refusals before anything is enqueued
    import torch
    d_x = torch.from_numpy(X.view(np.float32).reshape(-1).copy()).cuda()
    d_out = torch.full((int(np.prod(shapes["bands"])) + 8,), float("nan"), dtype=torch.float32, device="cuda")
    for bad in (dict(p=P(bands=17)), dict(T=7), dict(N=56), dict(bands=d_out.data_ptr() + 4), dict(bands=d_x.data_ptr() + 64)):
        ptr = dict(decorr=None, band_decorr=None, power=None, bands=d_out.data_ptr())
        ptr.update({k: v for k, v in bad.items() if k in ptr})
        p = bad.get("p", ssada.params(**good))
        rc = lib.fdoct_ssada(h, d_x.data_ptr(), DEV, bad.get("T", T), H, bad.get("N", N), p, ptr["decorr"], ptr["band_decorr"], ptr["power"], ptr["bands"], DEV)
        assert rc in (-1, -2), bad
    rec.synchronize()
    assert torch.isnan(d_out).all().item() and np.array_equal(d_x.cpu().numpy(), X.view(np.float32).reshape(-1))
    assert call() == 0   # ... and the handle works afterwards
    assert all(np.isfinite(a[:-2]).all() and np.isnan(a[-2:]).all() for a in outs.values())
    with pytest.raises(FdoctError):
        ssada.ssada(rec, X, good, want=("decorr", "decorr"))


# ---- 10. the physics -------------------------------------------------------------------------------------------------------------------
def test_the_moving_half_decorrelates_and_four_bands_calm_the_static_half(rec):
    """tests/ssada_cases.py: physics_field.  The model (tests/test_ssada_cases.py) shows the moving half's median decorrelation at
    4.2 (1 band) and 4.7 (4 bands) times the static half's, asserted at 2; and the static half's spread with 4 bands at 0.42 of its
    spread with 1 band at the same sigma, asserted at 0.75."""
    X = sc.physics_field()
    sc.physics_check({M: ssada.ssada(rec, X, dict(sc.PHYS, bands=M), want="decorr") for M in (1, 4)}, "the library")
