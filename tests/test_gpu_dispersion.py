"""GPU tests of the dispersion search (include/fdoct_dispersion.h; fdoct_amd/dispersion.py), held to tests/dispersion_model.py on the
fields and cases of tests/dispersion_cases.py: out_sums and out_row_sums against the composition in double by the project's
adjudication, the winner equal to the truth's, out_cos_sin within one float ulp of the winner's phase table; every subset of the
outputs the same bits as all four; NaN-poisoned outputs fully overwritten.  Then the invariants: every candidate of a 5 x 3 grid
searched again as a call of its own (the chunk seam), Parseval over the full depth range, device memory against host memory, NaN
rows, refusals that leave poisoned outputs alone, fdoct_process_dispersion_search against search() applied to what process_complex
returns, and both *_device functions behind a stall on the handle's stream against a quiet run (tests/stream_cases.py lists
Reconstructor methods only, so the stream-order check of these functions lives here).  The ratios of every case go to
helpers.TRUTH_LOG.

Measured on an MI355X (profiles/dispersion_ratios.txt): the worst |gpu - truth| / tol over the cases is 0.0184 for S2 and 0.0112 for
S4, where the float composition (scipy.fft on complex64) has 0.0105 and 0.0083: far inside the bound of 0.5, and below 0.1."""
import itertools

import numpy as np
import pytest

import dispersion_cases as dc
import dispersion_model as dm
import stream_stall as ss
from fdoct_amd import Config, FdoctError, Reconstructor, capi, dispersion, synth

pytestmark = pytest.mark.gpu

NAMES = dispersion.WANTS
POISON_BEST = np.array([(-77, -77, -77, -77, np.nan, np.nan, np.nan)], dispersion.BEST_DTYPE)


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage alone reads nothing of the geometry
    yield r
    r.close()


def _shapes(rows, K, n):
    return {"sums": (K, 2), "row_sums": (rows, K, 2), "cos_sin": (n, 2)}


def _poisoned(rows, K, n, want):
    outs = {}
    for w in want:
        if w == "best":
            outs[w] = POISON_BEST.copy()
        else:
            outs[w] = np.full(_shapes(rows, K, n)[w], np.nan, np.float32 if w == "cos_sin" else np.float64)
    return outs


def _untouched(outs):
    for w, a in outs.items():
        if w == "best":
            assert a.tobytes() == POISON_BEST.tobytes(), w
        else:
            assert np.isnan(a).all(), w


def _raw(rec, X, a2, a3, depth, want=NAMES, rows=None, n=None, g=None, K=None):
    """fdoct_dispersion_search itself on host memory with poisoned outputs: (return code, dict of the outputs)."""
    R, N = X.shape
    K = a2[2] * a3[2] if K is None else K
    outs = _poisoned(R, K, N, want)
    ptr = lambda w: outs[w].ctypes.data if w in outs else None   # noqa: E731
    g = dispersion.grid(a2, a3, depth) if g is None else g
    rc = rec.lib.fdoct_dispersion_search(rec.h, X.ctypes.data, capi.MEM_HOST, R if rows is None else rows, N if n is None else n, g, ptr("sums"),
                                         ptr("row_sums"), ptr("best"), ptr("cos_sin"), capi.MEM_HOST)
    return rc, outs


def _as_result(outs):
    """The raw outputs as check() takes them: best as a dict."""
    r = dict(outs)
    if "best" in r:
        b = r["best"][0]
        r["best"] = {k: (int(b[k]) if k in ("index", "i2", "i3") else float(b[k])) for k in ("index", "i2", "i3", "a2", "a3", "metric")}
    return r


@pytest.mark.parametrize("case", dc.CASES, ids=[c["what"] for c in dc.CASES])
def test_every_case_against_the_model(rec, case):
    X, a2, a3, depth = dc.case_field(case), case["a2"], case["a3"], case["depth"]
    t, f = dc.case_models(case)
    rc, full = _raw(rec, X, a2, a3, depth)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    for w in ("sums", "row_sums", "cos_sin"):
        assert np.isfinite(full[w]).all(), w + ": poison left"
    dm.check(_as_result(full), X, a2, a3, depth, case["what"], t, f)
    if case["recovery"]:
        assert full["best"]["index"][0] == dc.planted_index(case)
        assert (full["best"]["a2"][0], full["best"]["a3"][0]) == case["planted"]
    if case["zero_row"] is not None:
        assert np.all(full["row_sums"][case["zero_row"]] == 0)
    for k in (1, 2, 3):
        for want in itertools.combinations(NAMES, k):
            rc, part = _raw(rec, X, a2, a3, depth, want=want)
            assert rc == 0 and set(part) == set(want)
            for w in want:
                a, b = part[w], full[w]
                if w == "best":   # every field but the padding word
                    a, b = [a[k2] for k2 in ("index", "i2", "i3", "a2", "a3", "metric")], [b[k2] for k2 in ("index", "i2", "i3", "a2", "a3", "metric")]
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "best alone in %s" % (want,)
                else:
                    assert a.tobytes() == b.tobytes(), "%s alone in %s" % (w, want)
    got = dispersion.search(rec, X, a2, a3, depth)   # the binding returns the same
    for w in ("sums", "row_sums", "cos_sin"):
        assert got[w].tobytes() == full[w].tobytes(), w
    assert got["best"] == _as_result(full)["best"]
    one = dispersion.search(rec, X, a2, a3, depth, want="cos_sin")
    assert one.tobytes() == full["cos_sin"].tobytes()


def test_each_candidate_alone_gives_the_grid_s_bits(rec):
    """A 5 x 3 grid (two chunks of the plan: 8 and 7 candidates) against its 15 candidates as 1 x 1 calls: the chunk seam."""
    case = dc.CASES[1]
    X = dc.case_field(case)
    a2, a3, depth = (-4.0, 8.0, 5), (-6.0, 2.0, 3), case["depth"]
    p = dispersion.plan(a2, a3, X.shape[0], X.shape[1], depth)
    assert (p["candidates"], p["per_workgroup"], p["chunks"]) == (15, 8, 2)
    full = dispersion.search(rec, X, a2, a3, depth)
    for c in range(15):
        v2, v3 = dispersion.candidate(a2, a3, c)
        alone = dispersion.search(rec, X, (v2, 0.0, 1), (v3, 0.0, 1), depth)
        assert alone["row_sums"][:, 0].tobytes() == full["row_sums"][:, c].tobytes(), c
        assert alone["sums"][0].tobytes() == full["sums"][c].tobytes(), c
        assert alone["best"]["index"] == 0 and (alone["best"]["a2"], alone["best"]["a3"]) == (v2, v3)
        if c == full["best"]["index"]:
            assert alone["cos_sin"].tobytes() == full["cos_sin"].tobytes() and alone["best"]["metric"] == full["best"]["metric"]


def test_parseval_over_the_full_depth_range(rec):
    """Over every bin S2 is the row's energy whatever the candidate (|phasor| = 1), and at (0, 0) the A-scan is X itself."""
    case = dc.CASES[0]
    X, a2, a3 = dc.case_field(case), dc.A2, dc.A3
    n = X.shape[1]
    depth = (0, n)
    t = dm.model(X, a2, a3, depth, truth=True)
    tol_rows, tol_sums = dm.tolerances(t, n)
    got = dispersion.search(rec, X, a2, a3, depth, want=("sums", "row_sums"))
    s2 = got["sums"][:, 0]
    spread = np.abs(s2[:, None] - s2[None, :]) / (tol_sums[:, 0][:, None] + tol_sums[:, 0][None, :])
    c00 = 6 * a3[2] + 4
    assert dispersion.candidate(a2, a3, c00) == (0.0, 0.0)
    energy = (X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2).sum(-1)
    own = np.abs(got["row_sums"][:, c00, 0] - energy) / tol_rows[:, c00, 0]
    print("Parseval: worst |S2[c] - S2[c']| / (tol + tol') = %.4g; |S2[r][(0,0)] - sum|X|^2| / tol = %.4g" % (spread.max(), own.max()))
    assert spread.max() <= 1.0 and own.max() <= 1.0


def _busy_stream():
    """The caller's stream of the stalled runs: a high-priority one.  torch hands out the streams of its default pool in turn, and
    which two of them a later test gets decides whether they share a hardware queue (tests/test_gpu_stream_order.py's teeth check
    needs two that do not); taking from the other pool leaves that turn where it was."""
    import torch
    return torch.cuda.Stream(priority=-1)


def _device(rec, X, a2, a3, depth, want=NAMES, off=0, fill_on=None):
    """search_device on pairs in device memory into NaN-filled device memory, every output `off` bytes into its buffer."""
    import torch
    R, N = X.shape
    K = a2[2] * a3[2]
    sizes = {"sums": K * 16, "row_sums": R * K * 16, "best": 40, "cos_sin": N * 8}
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
    dispersion.search_device(rec, d_in.data_ptr(), R, N, a2, a3, ptr("sums"), ptr("row_sums"), ptr("best"), ptr("cos_sin"), depth=depth)
    if ev is not None:
        ss.still_running(ev, "search_device")
        fill_on.synchronize()
    rec.synchronize()
    return _device_outputs(bufs, sizes, want, off, R, K, N)


def _device_outputs(bufs, sizes, want, off, R, K, N):
    out = {}
    for w in NAMES:
        flat = bufs[w].cpu().numpy()
        k, size = off // 4, sizes[w] // 4
        if w in want:
            assert np.isnan(flat[:k]).all() and np.isnan(flat[k + size:]).all(), w + ": written outside the result"
            body = flat[k:k + size].copy()
            if w == "best":
                out[w] = body.view(dispersion.BEST_DTYPE)
            elif w == "cos_sin":
                out[w] = body.reshape(N, 2)
            else:
                out[w] = body.view(np.float64).reshape(_shapes(R, K, N)[w])
        else:
            assert np.isnan(flat).all()
    return out


def _best_fields(b):
    return tuple(b[k][0] for k in ("index", "i2", "i3", "a2", "a3", "metric"))


@pytest.mark.parametrize("case", [dc.CASES[2], dc.CASES[8]], ids=lambda c: c["what"])
def test_device_memory_gives_what_host_memory_gives(rec, case):
    X, a2, a3, depth = dc.case_field(case), case["a2"], case["a3"], case["depth"]
    rc, host = _raw(rec, X, a2, a3, depth)
    assert rc == 0
    dev = _device(rec, X, a2, a3, depth, off=8)
    for w in ("sums", "row_sums", "cos_sin"):
        assert dev[w].tobytes() == host[w].tobytes(), w
    assert _best_fields(dev["best"]) == _best_fields(host["best"])
    part = _device(rec, X, a2, a3, depth, want=("best", "cos_sin"))
    assert part["cos_sin"].tobytes() == host["cos_sin"].tobytes() and _best_fields(part["best"]) == _best_fields(host["best"])
    with pytest.raises(FdoctError) as e:       # 4 bytes off: refused, nothing written (the helper asserts that)
        _device(rec, X, a2, a3, depth, off=4)
    assert e.value.code == -1 and "8 bytes" in str(e.value)


def test_nan_rows(rec):
    case = dc.CASES[1]
    X0, a2, a3, depth = dc.case_field(case), case["a2"], case["a3"], case["depth"]
    clean = dispersion.search(rec, X0, a2, a3, depth)
    X = X0.copy()
    X[1, 5] = np.nan
    got = dispersion.search(rec, X, a2, a3, depth)
    assert np.isnan(got["row_sums"][1]).all()
    for r in (0, 2, 3):   # a NaN row poisons its own row sums only
        assert got["row_sums"][r].tobytes() == clean["row_sums"][r].tobytes(), r
    assert np.isnan(got["sums"]).all()   # ... and, through the sum over rows, every candidate's sums: no metric is finite
    assert got["best"] == dict(index=-1, i2=-1, i3=-1, a2=0.0, a3=0.0, metric=0.0) and np.all(got["cos_sin"] == 0)
    X[:] = np.nan
    rc, outs = _raw(rec, X, a2, a3, depth)
    assert rc == 0 and np.isnan(outs["sums"]).all() and np.isnan(outs["row_sums"]).all()
    assert _best_fields(outs["best"]) == (-1, -1, -1, 0.0, 0.0, 0.0) and np.all(outs["cos_sin"] == 0) and not np.isnan(outs["cos_sin"]).any()


def test_refusals_leave_poisoned_outputs_alone(rec):
    import torch
    X = dc.case_field(dc.CASES[1])
    a2, a3, depth = dc.A2, dc.A3, (2, 0)
    bad = [dict(a2=(0.0, 1.0, 0)), dict(a3=(0.0, 1.0, -2)), dict(a2=(float("nan"), 1.0, 13)), dict(a3=(0.0, float("inf"), 9)), dict(depth=(64, 0)),
           dict(depth=(0, 129)), dict(depth=(-1, 4)), dict(depth=(128, 1)), dict(rows=0), dict(rows=-3), dict(n=8), dict(n=0)]
    for kw in bad:
        rc, outs = _raw(rec, X, kw.get("a2", a2), kw.get("a3", a3), kw.get("depth", depth), rows=kw.get("rows"), n=kw.get("n"), K=117)
        assert rc == -1, kw
        _untouched(outs)
    for n in (112, 68):   # a prime factor above 5 (the buffer holds 4 x 128 pairs: more than either reads)
        rc, outs = _raw(rec, X, a2, a3, depth, rows=4, n=n)
        assert rc == -2, n
        _untouched(outs)
    big = np.zeros((1, 8192), np.complex64)
    rc, outs = _raw(rec, big, a2, a3, depth)
    assert rc == -2
    _untouched(outs)
    rc, outs = _raw(rec, X, (0.0, 1.0, 257), (0.0, 1.0, 256), depth, want=("best",))   # K beyond 65536
    assert rc == -1
    _untouched(outs)
    lib, g = rec.lib, dispersion.grid(a2, a3, depth)
    outs = _poisoned(4, 117, 128, NAMES)
    p = {w: outs[w].ctypes.data for w in NAMES}
    H = capi.MEM_HOST
    assert lib.fdoct_dispersion_search(rec.h, None, H, 4, 128, g, p["sums"], p["row_sums"], p["best"], p["cos_sin"], H) == -1
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, H, 4, 128, None, p["sums"], p["row_sums"], p["best"], p["cos_sin"], H) == -1
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, H, 4, 128, g, None, None, None, None, H) == -1
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, 7, 4, 128, g, p["sums"], p["row_sums"], p["best"], p["cos_sin"], H) == -1
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, H, 4, 128, g, p["sums"], p["row_sums"], p["best"], p["cos_sin"], 7) == -1
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data + 4, H, 3, 128, g, p["sums"], p["row_sums"], p["best"], p["cos_sin"], H) == -1
    for w in NAMES:   # each output 4 bytes off
        q = dict(p)
        q[w] += 4
        assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, H, 4, 128, g, q["sums"], q["row_sums"], q["best"], q["cos_sin"], H) == -1, w
    # overlaps: two outputs on each other, an output on the input
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, H, 4, 128, g, p["row_sums"] + 16, p["row_sums"], None, None, H) == -1
    assert lib.fdoct_dispersion_search(rec.h, X.ctypes.data, H, 4, 128, g, p["sums"], None, None, p["sums"] + 8, H) == -1
    Xw = X.copy()
    assert lib.fdoct_dispersion_search(rec.h, Xw.ctypes.data, H, 4, 128, g, None, None, None, Xw.ctypes.data + 1024, H) == -1
    assert Xw.tobytes() == X.tobytes()
    _untouched(outs)
    # ... and in device memory
    d = torch.full((4 * 128 * 2 + 4096,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(FdoctError) as e:
        dispersion.search_device(rec, d.data_ptr(), 4, 128, a2, a3, None, None, None, d.data_ptr() + 512)
    assert e.value.code == -1 and "overlap" in str(e.value)
    with pytest.raises(FdoctError) as e:
        dispersion.search_device(rec, d.data_ptr(), 4, 112, a2, a3, None, None, None, d.data_ptr() + 4 * 128 * 8)
    assert e.value.code == -2
    rec.synchronize()
    assert torch.isnan(d).all().item()


@pytest.fixture(scope="module")
def chain():
    W, H, N = 64, 4, 128
    frames = synth.make_frames(5, 2, W, H)
    yb = synth.make_background(W)
    full = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=N))
    full.set_background(yb)
    short = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=N // 2))
    short.set_background(yb)
    yield full, short, frames
    full.close()
    short.close()


def test_process_search_is_search_of_process_complex(chain):
    full, short, frames = chain
    a2, a3, depth = dc.A2, dc.A3, (2, 0)
    X = full.process_complex(frames)
    assert X.shape == (2, 4, 128) and np.isfinite(X.view(np.float32)).all()
    want = dispersion.search(full, X, a2, a3, depth)
    got = dispersion.process_search(full, frames, a2, a3, depth)
    for w in ("sums", "row_sums", "cos_sin"):
        assert got[w].tobytes() == want[w].tobytes(), w
    assert got["best"] == want["best"] and got["best"]["index"] >= 0
    assert got["row_sums"].shape == (8, 117, 2)
    one = dispersion.process_search(full, frames, a2, a3, depth, want="best")
    assert one == want["best"]
    # the table goes where it is meant to go: the instrument's handle takes it, and the call before it is unchanged
    before = full.process_complex(frames)
    assert before.tobytes() == X.tobytes()   # the search changed nothing a later call reads
    short.set_dispersion_phase(got["cos_sin"])
    short.set_dispersion_phase(None)
    # numdisplaypoints = 64: unsupported, outputs untouched
    outs = _poisoned(8, 117, 128, NAMES)
    g = dispersion.grid(a2, a3, depth)
    a = np.ascontiguousarray(frames)
    rc = short.lib.fdoct_process_dispersion_search(short.h, a.ctypes.data, capi._NP2DT[a.dtype], capi.MEM_HOST, 2, a.strides[1], g, outs["sums"].ctypes.data,
                                                   outs["row_sums"].ctypes.data, outs["best"].ctypes.data, outs["cos_sin"].ctypes.data, capi.MEM_HOST)
    assert rc == -2 and b"numdisplaypoints" in short.lib.fdoct_last_error(short.h)
    _untouched(outs)
    with pytest.raises(FdoctError) as e:
        dispersion.process_search(short, frames, a2, a3, depth)
    assert e.value.code == -2


def test_search_device_behind_a_stall_matches_a_quiet_run(rec):
    import torch
    case = dc.CASES[1]
    X, a2, a3, depth = dc.case_field(case), case["a2"], case["a3"], case["depth"]
    quiet = _device(rec, X, a2, a3, depth)   # (also the warm call: every workspace has its size)
    S = _busy_stream()
    rec.set_stream(S.cuda_stream)
    try:
        busy = _device(rec, X, a2, a3, depth, fill_on=S)
    finally:
        S.synchronize()
        rec.set_stream(None)
    for w in ("sums", "row_sums", "cos_sin"):
        assert busy[w].tobytes() == quiet[w].tobytes(), w
    assert _best_fields(busy["best"]) == _best_fields(quiet["best"]) and quiet["best"]["index"][0] == dc.planted_index(case)


def _process_device(full, frames, a2, a3, depth, fill_on=None):
    import torch
    n, H, W = frames.shape
    R, K, N = n * H, a2[2] * a3[2], 128
    sizes = {"sums": K * 16, "row_sums": R * K * 16, "best": 40, "cos_sin": N * 8}
    src = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()
    d_in = torch.zeros_like(src) if fill_on is not None else src
    bufs = {w: torch.full((sizes[w] // 4 + 8,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()
    ev = None
    if fill_on is not None:
        ev = ss.stall(fill_on)
        with torch.cuda.stream(fill_on):
            d_in.copy_(src, non_blocking=True)
    dispersion.process_search_device(full, d_in.data_ptr(), capi.DTYPE_U16, n, W * 2, a2, a3, bufs["sums"].data_ptr(), bufs["row_sums"].data_ptr(),
                                     bufs["best"].data_ptr(), bufs["cos_sin"].data_ptr(), depth=depth)
    if ev is not None:
        ss.still_running(ev, "process_search_device")
        fill_on.synchronize()
    full.synchronize()
    return _device_outputs(bufs, sizes, NAMES, 0, R, K, N)


def test_process_search_device_behind_a_stall_matches_a_quiet_run(chain):
    import torch
    full, _, frames = chain
    assert frames.dtype == np.uint16
    a2, a3, depth = dc.A2, dc.A3, (2, 0)
    host = dispersion.process_search(full, frames, a2, a3, depth)
    quiet = _process_device(full, frames, a2, a3, depth)
    for w in ("sums", "row_sums", "cos_sin"):
        assert quiet[w].tobytes() == host[w].tobytes(), w
    S = _busy_stream()
    full.set_stream(S.cuda_stream)
    try:
        busy = _process_device(full, frames, a2, a3, depth, fill_on=S)
    finally:
        S.synchronize()
        full.set_stream(None)
    for w in ("sums", "row_sums", "cos_sin"):
        assert busy[w].tobytes() == quiet[w].tobytes(), w
    assert _best_fields(busy["best"]) == _best_fields(quiet["best"]) == tuple(host["best"][k] for k in ("index", "i2", "i3", "a2", "a3", "metric"))
