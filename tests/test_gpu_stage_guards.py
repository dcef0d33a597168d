"""GPU tests of where the vibrometry stage and the dispersion search put outputs that go through the staging plan
(fdoct_amd/csrc/fdoct_stage.h): each output lies at an odd offset inside a larger NaN-filled buffer, in host or in device memory;
after the call every byte around it is what it was and the body holds the bytes of the all-device-memory call.  The shapes are
the smallest that give every output a size of its own, so that an output copied with another's size or to another's place
shows."""
import ctypes as C

import numpy as np
import pytest

import vibro_cases as vc
from fdoct_amd import Config, Reconstructor, capi, dispersion, vibrometry

pytestmark = pytest.mark.gpu

HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
SLACK = 64   # bytes behind every body


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stages alone read nothing of the geometry
    yield r
    r.close()


def _buffers(sizes, offs, space):
    """One NaN-filled buffer per output: `offs[w]` bytes, the body, SLACK bytes."""
    import torch
    bufs = {w: np.full((offs[w] + sizes[w] + SLACK) // 4, np.nan, np.float32) for w in sizes}
    return {w: torch.from_numpy(b).cuda() for w, b in bufs.items()} if space == DEVICE else bufs


def _addr(buf, off=0):
    return (buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data) + off


def _bodies(bufs, sizes, offs, written, what):
    """The bytes of every output in `written`, after checking that no byte outside them has changed."""
    out = {}
    for w, buf in bufs.items():
        raw = (buf.cpu().numpy() if hasattr(buf, "cpu") else buf).view(np.uint8)
        clean = np.full(raw.size // 4, np.nan, np.float32).view(np.uint8)
        guard = np.ones(raw.size, bool)
        if w in written:
            guard[offs[w]:offs[w] + sizes[w]] = False
            out[w] = raw[offs[w]:offs[w] + sizes[w]].tobytes()
        assert np.array_equal(raw[guard], clean[guard]), "%s: a byte outside %s was written" % (what, w)
    return out


def _input(X, space):
    import torch
    flat = np.ascontiguousarray(X).view(np.float32).reshape(-1).copy()
    return torch.from_numpy(flat).cuda() if space == DEVICE else flat


# ---- vibrometry: 4 frames x 3 A-scans x 5 depths, one frequency, one chunk --------------------------------------------------------------
VT, VH, VD = 4, 3, 5
V_SIZES = {"amp": VH * VD * 8, "rms": VH * VD * 4, "drift": VH * VD * 4, "power": VH * VD * 4}   # 120, 60, 60, 60
V_OFFS = {"amp": 24, "rms": 4, "drift": 12, "power": 20}   # odd multiples of 8 and of 4 bytes
V_KW = dict(freq=(0.25,), ref=(1, 2), detrend=1)


def _vibro(rec, X, space, out_space, what):
    import torch
    p = vibrometry.params(**V_KW)
    src = _input(X, space)
    bufs = _buffers(V_SIZES, V_OFFS, out_space)
    torch.cuda.synchronize()
    ptr = {w: _addr(bufs[w], V_OFFS[w]) for w in V_SIZES}
    rc = rec.lib.fdoct_vibro(rec.h, _addr(src), space, VT, VH, VD, C.byref(p), ptr["amp"], ptr["rms"], ptr["drift"], ptr["power"], out_space)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    rec.synchronize()
    return _bodies(bufs, V_SIZES, V_OFFS, set(V_SIZES), what)


def test_vibro_outputs_land_where_the_caller_put_them(rec):
    X = vc.field(VT, VH, VD, 11, surface=(1, 2), common=1.0)
    assert vibrometry.plan(V_KW, VT, VH, VD)["chunks"] == 1
    want = _vibro(rec, X, DEVICE, DEVICE, "device memory")
    for w in V_SIZES:
        assert np.isfinite(np.frombuffer(want[w], np.float32)).all(), w
    assert np.count_nonzero(np.frombuffer(want["amp"], np.float32)) > 0
    for space, out_space, what in ((HOST, HOST, "host memory"), (DEVICE, HOST, "device pairs, host outputs"), (HOST, DEVICE, "host pairs, device outputs")):
        got = _vibro(rec, X, space, out_space, what)
        for w in V_SIZES:
            assert got[w] == want[w], "%s: %s" % (what, w)


# ---- the dispersion search: 2 rows of 16 points, a 3 x 1 grid ----------------------------------------------------------------------------
DR, DN, A2, A3 = 2, 16, (-4.0, 4.0, 3), (0.0, 1.0, 1)
D_SIZES = {"sums": 3 * 16, "row_sums": DR * 3 * 16, "best": dispersion.BEST_DTYPE.itemsize, "cos_sin": DN * 8}   # 48, 96, 40, 128
D_OFFS = {"sums": 8, "row_sums": 24, "best": 40, "cos_sin": 56}   # odd multiples of 8 bytes
D_NAMES = dispersion.WANTS


def _search(rec, X, space, out_space, want, what):
    import torch
    g = dispersion.grid(A2, A3)
    src = _input(X, space)
    bufs = _buffers(D_SIZES, D_OFFS, out_space)
    torch.cuda.synchronize()
    ptr = {w: _addr(bufs[w], D_OFFS[w]) if w in want else None for w in D_NAMES}
    rc = rec.lib.fdoct_dispersion_search(rec.h, _addr(src), space, DR, DN, C.byref(g), ptr["sums"], ptr["row_sums"], ptr["best"], ptr["cos_sin"], out_space)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    rec.synchronize()
    got = _bodies(bufs, D_SIZES, D_OFFS, set(want), what)
    if "best" in got:   # every field but the padding word, which the kernel does not write
        got["best"] = got["best"][:12] + got["best"][16:]
    return got


def test_dispersion_outputs_land_where_the_caller_put_them(rec):
    assert D_SIZES == {"sums": 48, "row_sums": 96, "best": 40, "cos_sin": 128}
    rng = np.random.default_rng(23)
    X = (rng.normal(0, 100, (DR, DN)) + 1j * rng.normal(0, 100, (DR, DN))).astype(np.complex64)
    full = _search(rec, X, DEVICE, DEVICE, D_NAMES, "device memory")
    assert np.isfinite(np.frombuffer(full["sums"], np.float64)).all() and np.isfinite(np.frombuffer(full["row_sums"], np.float64)).all()
    assert np.isfinite(np.frombuffer(full["cos_sin"], np.float32)).all()
    best = np.frombuffer(full["best"][:12], np.int32)
    assert 0 <= best[0] < 3 and best[1] == best[0] and best[2] == 0 and np.isfinite(np.frombuffer(full["best"][12:], np.float64)).all()
    host = _search(rec, X, HOST, HOST, D_NAMES, "host memory")
    for w in D_NAMES:
        assert host[w] == full[w], "host memory: " + w
    alone = _search(rec, X, HOST, HOST, ("best",), "the winner alone, host memory")
    assert alone["best"] == full["best"]
    rest = _search(rec, X, DEVICE, DEVICE, ("sums", "row_sums", "cos_sin"), "device memory, no winner")
    for w in rest:
        assert rest[w] == full[w], "device memory, no winner: " + w
