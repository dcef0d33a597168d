"""GPU tests of include/fdoct_saveframes.h against tests/saveframes_model.py.
  pictures     equal the model's bytes exactly, no pixel left out: test_saveframes_model.py shows that no pixel of the shared
               inputs lies within tie_band of a rounding tie, so the last bits of the device's double log cannot decide a byte
  out_bscan    bit for bit: the double sums in frame order, the IEEE division, the add of eps and the one rounding to float are
               all determined
  out_db       at most one float ulp from the model (the rule of test_gpu_manualavg.py): the device's double log and NumPy's may
               differ in their last double bits, and two doubles that close round to equal or adjacent floats
  raw switch   np.float32(raw) + np.float32(eps) against the default run of every kernel family
The launches (fdoct_saveframes.hip): 256 threads per workgroup; the scan takes 4096 elements of an image at a time, at most 256
workgroup columns per image and 2 x resident workgroups in all; the picture pass works on 64 x 64 tiles (H x D input) or
4096-element chunks (D x H input), at most 2 x resident workgroups."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import saveframes_model as m
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
HXD, DXH = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
INVALID, UNSUPPORTED = -1, -2      # FDOCT_ERR_INVALID, FDOCT_ERR_UNSUPPORTED (include/fdoct.h)
assert (HXD, DXH) == (m.ROWMAJOR, m.TRANSPOSED)


def _handle(variant=capi.VARIANT_MAIN, dc_mask=1):
    return Reconstructor(Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128, variant=variant, dc_mask=dc_mask))


@pytest.fixture(scope="module")
def rec():
    r = _handle()
    yield r
    r.close()


@pytest.fixture(scope="module")
def rec_nomask():
    r = _handle(dc_mask=0)
    yield r
    r.close()


class _Canary:
    """A device buffer of n bytes that starts `offset` bytes behind a 16-byte boundary, filled with 0xA5 like the 32 + offset
    bytes in front of it and the 32 behind it."""
    GUARD = 32

    def __init__(self, n, offset=0):
        import torch
        self.n, self.at = n, self.GUARD + offset
        self.t = torch.full((self.at + n + self.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.at

    def load(self, a):
        import torch
        self.t[self.at:self.at + self.n] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()

    def bytes(self):
        a = self.t.cpu().numpy()
        assert (a[:self.at] == 0xA5).all() and (a[self.at + self.n:] == 0xA5).all(), "bytes outside the buffer were written"
        return a[self.at:self.at + self.n]

    def untouched(self):
        return bool((self.t == 0xA5).all().item())


def _ordered(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return int(np.abs(_ordered(a) - _ordered(b)).max()) if a.size else 0


def _device_call(r, frames, il, averages=0, ol=DXH, want=(True, True, True), src_off=0, gray_off=0, fold_off=0):
    """fdoct_saveframes on device memory: frames float32 (n, rows, cols) in il -> (gray, bscan, db) as numpy (None where not
    wanted).  The offsets shift the source (floats), the pictures (bytes) and the fold outputs (floats) off their 16-byte
    boundaries; every buffer lies between 0xA5 canaries, and the source must come back as it went."""
    import torch
    n, rows, cols = frames.shape
    D, H = (rows, cols) if il == DXH else (cols, rows)
    G = n // averages if averages else 0
    src = _Canary(frames.size * 4, 4 * src_off)
    src.load(frames)
    gray = _Canary(n * D * H, gray_off) if want[0] else None
    mag = _Canary(G * D * H * 4, 4 * fold_off) if want[1] and G else None
    db = _Canary(G * D * H * 4, 4 * fold_off) if want[2] and G else None
    torch.cuda.synchronize()
    r.saveframes_device(src.ptr, n, D, H, gray.ptr if gray else None, averages, mag.ptr if mag else None, db.ptr if db else None, il, ol)
    r.synchronize()
    assert np.array_equal(src.bytes(), frames.reshape(-1).view(np.uint8)), "the input was written"
    shp = (G, D, H) if ol == DXH else (G, H, D)
    return (gray.bytes().reshape(n, D, H) if gray else None, mag.bytes().view(np.float32).reshape(shp) if mag else None,
            db.bytes().view(np.float32).reshape(shp) if db else None)


def _model_pictures(frames_hd):
    return np.stack([m.image(f, m.ROWMAJOR) for f in frames_hd])


# ---- pictures

@pytest.mark.parametrize("il", [HXD, DXH])
@pytest.mark.parametrize("shape", m.PICTURE_SHAPES)
def test_pictures_equal_the_model_byte_for_byte(rec, shape, il):
    """One and three frames with different content per frame: extrema in the first and last pixel, extrema inside the last
    partial tile, zeros anywhere."""
    H, D = shape
    sets = [m.frames_hd(shape, 3)] + [m.frames_hd(shape, 1, first=k) for k in range(3)]
    for f in sets:
        want = _model_pictures(f)
        gray, _, _ = _device_call(rec, m.in_layout_of(f, il), il)
        assert gray.shape == (f.shape[0], D, H)
        bad = np.argwhere(gray != want)
        assert bad.size == 0, "shape %s layout %d, %d frame(s): %d bytes differ, first at %s: %d, model %d" % (
            shape, il, f.shape[0], len(bad), bad[0], gray[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("il", [HXD, DXH])
def test_an_image_beyond_every_cap(rec, il):
    """1025 x 1024 pixels: more than 256 partial extrema x 4096 pixels, so every workgroup column of the scan takes a second
    chunk and folds its extrema into the pair it wrote before -- and the image's extrema sit among the pixels only that second
    round reaches (H x D order; in D x H order the maximum does)."""
    f = m.frames_hd(m.BIG_SHAPE, 1, first=1)
    gray, _, _ = _device_call(rec, m.in_layout_of(f, il), il)
    assert np.array_equal(gray, _model_pictures(f))


def test_more_images_than_either_grid_holds(rec):
    """5000 images of 1 x 7 pixels: the scan's grid holds at most 2 x resident groups and the picture pass's as many work items;
    both sweep the rest in their loops.  With the fold over groups of one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 5000
    assert n > 2 * cus * 4          # 2 x resident_blocks(CUs, 16 waves per CU, 256)
    f = m.frames_hd((1, 7), n)
    for il in (HXD, DXH):
        gray, b, db = _device_call(rec, m.in_layout_of(f, il), il, averages=1, ol=il)
        assert np.array_equal(gray, _model_pictures(f))
        want_b, want_db = m.fold(m.in_layout_of(f, il), 1, m.EPS_MAIN, 1, il, il)
        assert np.array_equal(b.view(np.uint32), want_b.view(np.uint32)) and _ulps(db, want_db) <= 1


@pytest.mark.parametrize("il", [HXD, DXH])
def test_constant_and_zero_images_give_zeros(rec, il):
    f = np.stack([np.full((67, 129), 3.25, np.float32), np.zeros((67, 129), np.float32), m.frames_hd((67, 129), 1, first=2)[0]])
    gray, _, _ = _device_call(rec, m.in_layout_of(f, il), il)
    assert not gray[0].any() and not gray[1].any()
    assert np.array_equal(gray[2], m.image(f[2], m.ROWMAJOR)) and gray[2].max() == 255


# ---- fold

FOLD_SHAPES = [(6, 4), (6, 5), (66, 64), (67, 129)]      # (H, D): depths 4 and 5 at the DC mask's edge; 16-byte and element-wise scans of two and three chunks


@pytest.mark.parametrize("averages,n", [(1, 5), (3, 15), (5, 5), (5, 15)])
@pytest.mark.parametrize("shape", FOLD_SHAPES)
def test_fold_equals_the_model_in_every_layout_pair(rec, rec_nomask, shape, averages, n):
    H, D = shape
    f = m.fold_frames(n, H, D)
    for dc, r in ((1, rec), (0, rec_nomask)):
        first = None
        for il in (HXD, DXH):
            for ol in (HXD, DXH):
                want_b, want_db = m.fold(m.in_layout_of(f, il), averages, m.EPS_MAIN, dc, il, ol)
                _, b, db = _device_call(r, m.in_layout_of(f, il), il, averages, ol, want=(False, True, True))
                what = "shape %s averages %d n %d dc %d layouts %d -> %d" % (shape, averages, n, dc, il, ol)
                assert np.array_equal(b.view(np.uint32), want_b.view(np.uint32)), what + ": out_bscan differs from the model"
                assert _ulps(db, want_db) <= 1, what + ": out_db %d ulp from the model" % _ulps(db, want_db)
                if ol == HXD:
                    b, db = np.transpose(b, (0, 2, 1)), np.transpose(db, (0, 2, 1))
                if first is None:
                    first = (b.copy(), db.copy())
                assert np.array_equal(b.view(np.uint32), first[0].view(np.uint32)), what + ": layout pairs differ"
                assert np.array_equal(db.view(np.uint32), first[1].view(np.uint32)), what + ": layout pairs differ"
        if dc and D > 4:
            assert np.array_equal(first[1][:, 0], first[1][:, 4]) and np.array_equal(first[1][:, 1], first[1][:, 4])
            assert not np.array_equal(first[0][:, 0], first[0][:, 4])          # the linear image carries no mask


def test_pictures_and_fold_in_one_call_and_each_output_alone(rec):
    f = m.frames_hd((67, 129), 3)
    want_gray = _model_pictures(f)
    want_b, want_db = m.fold(f, 3, m.EPS_MAIN, 1, m.ROWMAJOR, m.TRANSPOSED)
    gray, b, db = _device_call(rec, f, HXD, 3)
    assert np.array_equal(gray, want_gray) and np.array_equal(b.view(np.uint32), want_b.view(np.uint32)) and _ulps(db, want_db) <= 1
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        g2, b2, d2 = _device_call(rec, f, HXD, 3, want=want)
        for got, ref in ((g2, gray), (b2, b), (d2, db)):
            assert got is None or np.array_equal(got.view(np.uint8), ref.view(np.uint8)), want
    g3, b3, d3 = _device_call(rec, f, HXD, 3, want=(True, False, False))    # averages given, no fold output: pictures alone
    assert b3 is None and d3 is None and np.array_equal(g3, gray)


def test_the_sim_variant_has_pictures_and_no_fold():
    import torch
    sim = _handle(variant=capi.VARIANT_SIM)
    f = m.frames_hd((3, 85), 3)
    gray, _, _ = _device_call(sim, f, HXD)
    assert np.array_equal(gray, _model_pictures(f))
    out = torch.full((3 * 85,), -7.0, dtype=torch.float32, device="cuda")
    src = torch.from_numpy(f.copy()).cuda()
    torch.cuda.synchronize()
    with pytest.raises(FdoctError) as e:
        sim.saveframes_device(src.data_ptr(), 3, 85, 3, None, 3, out.data_ptr(), None)
    # (FDOCT_ERR_UNSUPPORTED is -2 in include/fdoct.h; -3 is FDOCT_ERR_DEVICE)
    assert e.value.code == UNSUPPORTED and "sim" in str(e.value) and bool((out == -7.0).all().item())
    sim.close()


# ---- pointers

@pytest.mark.parametrize("il", [HXD, DXH])
@pytest.mark.parametrize("which", ["aligned", "src", "gray1", "gray3", "fold", "all"])
def test_misaligned_device_pointers(rec, which, il):
    """68 x 64 pixels: count and ascans are multiples of four, so only the pointers decide between the 16-byte loads and 4-byte
    stores and the element-wise ones.  The source off by one float, the pictures by one and by three bytes, the fold outputs by
    one float, each alone and all together: the model's results, between canaries that keep their 0xA5."""
    f = m.frames_hd((68, 64), 3)
    want_gray = _model_pictures(f)
    want_b, want_db = m.fold(f, 3, m.EPS_MAIN, 1, m.ROWMAJOR, m.TRANSPOSED)
    off = dict(src_off=1 if which in ("src", "all") else 0, gray_off={"gray1": 1, "gray3": 3, "all": 3}.get(which, 0),
               fold_off=1 if which in ("fold", "all") else 0)
    gray, b, db = _device_call(rec, m.in_layout_of(f, il), il, 3, **off)
    assert np.array_equal(gray, want_gray), which
    assert np.array_equal(b.view(np.uint32), want_b.view(np.uint32)) and _ulps(db, want_db) <= 1, which


def test_the_host_memory_call_equals_the_device_call(rec):
    f = m.frames_hd((67, 129), 3)
    for il in (HXD, DXH):
        x = m.in_layout_of(f, il)
        dev = _device_call(rec, x, il, 3)
        host = rec.saveframes(x, 3, il, DXH)
        for a, b in zip(dev, host):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    g, b, db = rec.saveframes(f[0], 0)                  # one image, no fold
    assert g.shape == (1, 129, 67) and b is None and db is None and np.array_equal(g[0], m.image(f[0], m.ROWMAJOR))


# ---- refusals on the device

def test_overlaps_are_refused_and_touch_nothing(rec):
    f = m.frames_hd((16, 12), 3)
    n, count = 3, 16 * 12
    src = _Canary(n * count * 4)
    src.load(f)
    gray, mag, db = _Canary(n * count), _Canary(count * 4), _Canary(count * 4)
    lib, h = rec.lib, rec.h

    def call(g=gray.ptr, b=mag.ptr, d=db.ptr, mem=DEVICE):
        import torch
        torch.cuda.synchronize()
        return lib.fdoct_saveframes(h, src.ptr, DEVICE, HXD, n, 12, 16, g, 3, b, d, DXH, mem)

    for bad in (dict(g=src.ptr + 4 * (n * count - 1)),            # the pictures begin on the input's last float
                dict(b=src.ptr + 4 * (n * count - 1)),            # ... the linear image does
                dict(d=src.ptr), dict(d=mag.ptr + 4 * (count - 1)),  # the outputs on each other
                dict(g=mag.ptr + 4 * count - 1), dict(b=gray.ptr + 4)):
        assert call(**bad) == INVALID, bad
        assert b"overlap" in lib.fdoct_last_error(h), bad
    assert call(g=None, b=None, d=None) == INVALID and b"no output" in lib.fdoct_last_error(h)
    rec.synchronize()
    assert gray.untouched() and mag.untouched() and db.untouched()
    assert np.array_equal(src.bytes(), f.reshape(-1).view(np.uint8))
    assert call() == 0                                              # and the same call made correctly goes through
    rec.synchronize()
    want_b, want_db = m.fold(f, 3, m.EPS_MAIN, 1, m.ROWMAJOR, m.TRANSPOSED)
    assert np.array_equal(gray.bytes().reshape(n, 12, 16), _model_pictures(f))
    assert np.array_equal(mag.bytes().view(np.uint32), want_b.reshape(-1).view(np.uint32))
    assert _ulps(db.bytes().view(np.float32), want_db.reshape(-1)) <= 1


# ---- raw magnitudes

FAMILIES = [
    ("fused", dict(width=2048, height=16, numfftpoints=2048, numdisplaypoints=1024), None, HXD, capi.KERNEL_FUSED),
    ("fused, D x H", dict(width=2048, height=16, numfftpoints=2048, numdisplaypoints=1024), None, DXH, capi.KERNEL_FUSED_TRANSPOSED),
    ("fused, staged", dict(width=2048, height=16, numfftpoints=2048, numdisplaypoints=1024), lambda r: r.set_staged(True), HXD, capi.KERNEL_FUSED_STAGED),
    ("wave", dict(width=160, height=16, numfftpoints=2560, numdisplaypoints=320, increasefftpointsmultiplier=4), None, HXD, capi.KERNEL_WAVE),
    ("wave, run-time compiled", dict(width=200, height=6, numfftpoints=2560, numdisplaypoints=320, increasefftpointsmultiplier=4,
                                     lambdamin=840.5e-9, lambdamax=859.5e-9), None, HXD, capi.KERNEL_WAVE_JIT),
    ("generic", dict(width=2048, height=16, numfftpoints=2002, numdisplaypoints=1001), None, HXD, capi.KERNEL_GENERIC),
    ("long rows", dict(width=2048, height=3, numfftpoints=65536, numdisplaypoints=2048, increasefftpointsmultiplier=8), None, HXD, capi.KERNEL_LONG_ROWS),
]


@pytest.mark.parametrize("name,cfg_kw,setup,layout,family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_raw_magnitudes_are_the_default_output_without_its_epsilon(name, cfg_kw, setup, layout, family):
    cfg = Config(**cfg_kw)
    r = Reconstructor(cfg)
    r.set_background(synth.make_background(cfg.width))
    if setup:
        setup(r)
    frames = synth.make_frames(0, 6, cfg.width, cfg.height)
    eps = np.float32(1e-5)
    assert r.get_raw_magnitudes() is False
    base1, db1 = r.process(frames[:2], layout=layout)
    assert r.last_kernel() == family, (name, r.last_kernel(), r.jit_note())
    r.set_raw_magnitudes(True)
    assert r.get_raw_magnitudes() is True
    raw1, none = r.process(frames[:2], want_db=False, layout=layout)
    assert none is None and r.last_kernel() == family
    # averages = 1: fmaf(acc, 1, eps) is one correctly rounded add, and so is NumPy's
    assert np.array_equal((raw1 + eps).view(np.uint32), base1.view(np.uint32)), name
    assert (raw1 >= 0).all() and not np.array_equal(raw1, base1)
    # a dB output with the switch on: refused, nothing written
    mag, db = np.full_like(base1, -7.0), np.full_like(base1, -7.0)
    with pytest.raises(FdoctError) as e:
        r.process(frames[:2], layout=layout, out_bscan=mag, out_db=db)
    assert e.value.code == INVALID and "out_db" in str(e.value) and (mag == -7.0).all() and (db == -7.0).all()
    import torch
    d_frames = torch.from_numpy(frames[:2].view(np.int16)).cuda()
    d_out = torch.full((2,) + base1.shape, -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(FdoctError) as e:
        r.process_device(d_frames.data_ptr(), capi.DTYPE_U16, 2, 0, d_out[0].data_ptr(), d_out[1].data_ptr(), layout)
    r.synchronize()
    assert e.value.code == INVALID and bool((d_out == -7.0).all().item())
    # a clone carries the switch
    twin = r.clone_to_device(0)
    assert twin.get_raw_magnitudes() is True
    assert np.array_equal(twin.process(frames[:2], want_db=False, layout=layout)[0].view(np.uint32), raw1.view(np.uint32))
    twin.close()
    # averages = 3: the default is fmaf(acc, 1/3, eps) rounded once, the sum from the raw output is rounded twice
    r.set_averages(3)
    raw3, _ = r.process(frames, want_db=False, layout=layout)
    r.set_raw_magnitudes(False)
    base3, _ = r.process(frames, layout=layout)
    assert raw3.shape == base3.shape and raw3.shape[0] == 2
    assert _ulps(raw3 + eps, base3) <= 1, "%s: %d ulp" % (name, _ulps(raw3 + eps, base3))
    # switched off again: what it was before, bit for bit
    r.set_averages(1)
    again, db_again = r.process(frames[:2], layout=layout)
    assert np.array_equal(again.view(np.uint32), base1.view(np.uint32)) and np.array_equal(db_again.view(np.uint32), db1.view(np.uint32))
    r.close()


def test_the_binning_keeps_its_epsilon_with_the_switch_on(rec):
    """fdoct_bscan_bin clamps at the variant's epsilon whatever the chain writes (chain_eps, not kernel_eps)."""
    b = np.zeros((1, 8, 8), np.float32)
    want = rec.bscan_bin(b, 2, 2)
    rec.set_raw_magnitudes(True)
    got = rec.bscan_bin(b, 2, 2)
    rec.set_raw_magnitudes(False)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.isfinite(got[1]).all()


# ---- end to end

E2E = dict(W=1024, H=8, N=1024, D=512, A=4, n=8)
_E2E = {}


def _e2e():
    """The chain once per frame (averages = 1, raw magnitudes) and fdoct_saveframes on its output where it lies; computed once."""
    if not _E2E:
        import torch
        W, H, N, D, A, n = (E2E[k] for k in "W H N D A n".split())
        frames, yb = synth.make_frames(0, n, W, H), synth.make_background(W)
        r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, averages=1))
        r.set_background(yb)
        r.set_raw_magnitudes(True)
        d_frames = torch.from_numpy(frames.view(np.int16)).cuda()
        d_mag = torch.empty((n, H, D), dtype=torch.float32, device="cuda")
        d_gray = torch.empty((n, D, H), dtype=torch.uint8, device="cuda")
        d_b, d_db = torch.empty((n // A, D, H), dtype=torch.float32, device="cuda"), torch.empty((n // A, D, H), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.process_device(d_frames.data_ptr(), capi.DTYPE_U16, n, 0, d_mag.data_ptr(), None, HXD)
        r.saveframes_device(d_mag.data_ptr(), n, D, H, d_gray.data_ptr(), A, d_b.data_ptr(), d_db.data_ptr(), HXD, DXH)
        r.synchronize()
        r.close()
        _E2E.update(frames=frames, yb=yb, mag=d_mag.cpu().numpy(), gray=d_gray.cpu().numpy(), b=d_b.cpu().numpy(), db=d_db.cpu().numpy())
    return _E2E


def test_chain_then_saveframes_on_device_memory():
    e = _e2e()
    W, H, N, D, A, n = (E2E[k] for k in "W H N D A n".split())
    assert np.array_equal(e["gray"], _model_pictures(e["mag"])), "pictures differ from the model applied to the chain's own output"
    want_b, want_db = m.fold(e["mag"], A, m.EPS_MAIN, 1, m.ROWMAJOR, m.TRANSPOSED)
    assert np.array_equal(e["b"].view(np.uint32), want_b.view(np.uint32)) and _ulps(e["db"], want_db) <= 1
    # against the oracle's chain with averages = 4: the project's rule, |gpu - truth| <= max(0.5 x tolerance, the f32
    # restatement's own distance), for the linear image and, through the dB tolerance the linear one implies, for bscandb
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, averages=A)
    mag_o, _, db_o = helpers.oracle_reference(cfg, e["frames"], e["yb"])
    mag_t, _, db_t = helpers.oracle_truth(cfg, e["frames"], e["yb"])
    g_lin, o_lin = helpers.check_truth(np.transpose(e["b"], (0, 2, 1)), mag_t, mag_o, "saveframes fold, linear")
    hd = lambda x: np.transpose(x, (0, 2, 1))
    g_db = float(helpers.db_ratio(hd(e["db"]), hd(db_t), mag_t).max())
    o_db = float(helpers.db_ratio(hd(db_o), hd(db_t), mag_t).max())
    print("fold against the chain in double: linear %.3f (f32 oracle %.3f), dB %.3f (f32 oracle %.3f) of the tolerance" % (g_lin, o_lin, g_db, o_db))
    assert np.isfinite(e["db"]).all() and g_db <= max(helpers.TRUTH_LIMIT, o_db)


def test_host_harness_writes_the_pictures_and_the_averaged_bscans(tmp_path):
    """host/bscanfft_sim --save-frames --averages 4 on the same frames: <prefix>_bscanNNN-III.pgm equal the pictures of the
    device-memory route, and the averaged B-scans it writes are that route's fold."""
    e = _e2e()
    W, H, N, D, A, n = (E2E[k] for k in "W H N D A n".split())
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    (tmp_path / "f.bin").write_bytes(e["frames"].tobytes())
    (tmp_path / "b.bin").write_bytes(e["yb"].tobytes())
    prefix = str(tmp_path / "out")
    cmd = [os.path.join(ROOT, "host", "bscanfft_sim"), "--frames", str(tmp_path / "f.bin"), "--background", str(tmp_path / "b.bin"),
           "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N), "--numdisplaypoints", str(D),
           "--averages", str(A), "--out", prefix, "--save-frames"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    header = b"P5\n%d %d\n255\n" % (H, D)
    for f in range(n):
        data = open("%s_bscan%03d-%03d.pgm" % (prefix, f // A + 1, f % A), "rb").read()
        assert data[:len(header)] == header
        assert np.array_equal(np.frombuffer(data[len(header):], np.uint8).reshape(D, H), e["gray"][f]), f
    assert not os.path.exists("%s_bscan%03d-%03d.pgm" % (prefix, n // A + 1, 0))
    assert np.array_equal(np.fromfile(prefix + "_bscan.f32", np.float32).view(np.uint32), e["b"].reshape(-1).view(np.uint32))
    assert np.array_equal(np.fromfile(prefix + "_bscandb.f32", np.float32).view(np.uint32), e["db"].reshape(-1).view(np.uint32))
    bad = subprocess.run(cmd + ["--sim"], capture_output=True, text=True, timeout=240)
    assert bad.returncode != 0 and "sim" in bad.stderr
