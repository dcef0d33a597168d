"""GPU tests of the reference-frame capture (include/fdoct_capture.h) against tests/capture_model.py, the recipe of the
reference's b / p / dark key handlers composed from the oracle's restatements.  Every comparison is bit for bit on the
doubles (as uint64 words, so that a sign of zero counts): the sums are exact for integer samples, run in the reference's
order for float samples, and the normalisations use the oracle's arithmetic.  There is no tolerance anywhere."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import capture_model
from capture_model import BACKGROUND, DARK, NONE, PI, bits
from fdoct_amd import VARIANT_SIM, Config, FdoctError, Reconstructor, capi, io, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32, "f64": np.float64}


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), what


def _frames(dtype, n, H, W, seed):
    """n frames of H x W: the golden backg fixture (tiled to the geometry) plus seeded noise; float frames carry non-integer
    samples."""
    rng = np.random.default_rng(seed)
    backg = np.fromfile(os.path.join(GOLD, "backg_u16_96x128.bin"), np.uint16).reshape(96, 128).astype(np.float64)
    base = np.tile(backg, ((H + 95) // 96, (W + 127) // 128))[:H, :W]
    noisy = base[None] * rng.uniform(0.6, 0.9, (n, 1, 1)) + rng.normal(0.0, 300.0, (n, H, W))
    dt = np.dtype(dtype)
    if dt == np.uint16:
        return np.clip(np.rint(noisy), 0, 65535).astype(np.uint16)
    if dt == np.uint8:
        return np.clip(np.rint(noisy / 256.0), 0, 255).astype(np.uint8)
    return (noisy / 7.0 + rng.random((n, H, W))).astype(dt)


class _DeviceFrames:
    """Frames in device memory at a row pitch of `pad` samples more than a row, `offset` samples past a 16-byte boundary."""

    def __init__(self, frames, pad=0, offset=0):
        import torch
        n, r, c = frames.shape
        es = frames.dtype.itemsize
        padded = np.zeros((n, r, c + pad), frames.dtype)
        padded[:, :, :c] = frames
        raw = np.zeros(offset * es + padded.nbytes, np.uint8)
        raw[offset * es:] = padded.view(np.uint8).ravel()
        self.t = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + offset * es
        self.pitch = (c + pad) * es
        self.dtype = capi._NP2DT[frames.dtype]
        self.n = n


def _host_view(frames, pad):
    """The same frames in host memory with padded rows (a view: its pitch goes to the library)."""
    n, r, c = frames.shape
    padded = np.zeros((n, r, c + pad), frames.dtype)
    padded[:, :, :c] = frames
    return padded[:, :, :c]


def _capture(rec, role, frames, device, pad=0, offset=0):
    if device:
        d = _DeviceFrames(frames, pad, offset)
        return rec.capture_reference_device(role, d.ptr, d.dtype, d.n, d.pitch, out=True)
    return rec.capture_reference(role, _host_view(frames, pad) if pad else frames, out=True)


GEOM = {"gold": dict(width=128, height=96, numfftpoints=1024, numdisplaypoints=512),
        "odd": dict(width=200, height=6, numfftpoints=2560, numdisplaypoints=320, increasefftpointsmultiplier=4)}


def _recipe_cases():
    """dtype x (donotnormalize, rowwisenormalize) x movavgn in full; host / device frames and nframes are laid over that
    product by the sum of the three indices, so that every value of any one option meets every value of any other one (checked
    below: a pairing that ties two options together would hide a path)."""
    flags, movs, counts = [(1, 0), (0, 0), (1, 1), (0, 1)], [0, 2, 3], (1, 3, 16)
    rows = []
    for (di, dt), (fi, (dnn, rwn)), (mi, mov) in itertools.product(enumerate(DTYPES), enumerate(flags), enumerate(movs)):
        s = di + fi + mi
        rows.append((dt, dnn, rwn, mov, s % 2, counts[s % 3]))
    options = [lambda r: r[0], lambda r: (r[1], r[2]), lambda r: r[3], lambda r: r[4], lambda r: r[5]]
    for a, b in itertools.combinations(options, 2):
        seen = {(a(r), b(r)) for r in rows}
        assert len(seen) == len({a(r) for r in rows}) * len({b(r) for r in rows}), "two options of the matrix are tied together"
    return [pytest.param(*r, id="%s-dnn%d-rwn%d-mov%d-%s-n%d" % (r[0], r[1], r[2], r[3], "dev" if r[4] else "host", r[5])) for r in rows]


@pytest.mark.parametrize("geom", ["gold", "odd"])
@pytest.mark.parametrize("dt,dnn,rwn,mov,device,nframes", _recipe_cases())
def test_every_role_matches_the_model_bit_for_bit(geom, dt, dnn, rwn, mov, device, nframes):
    g = GEOM[geom]
    W, H = g["width"], g["height"]
    # the odd geometry: a pitch larger than the row, and (device frames) a pointer one sample past a 16-byte boundary
    pad, offset = (5, 1) if geom == "odd" else (0, 0)
    rec = Reconstructor(Config(rowwisenormalize=rwn, donotnormalize=dnn, movavgn=mov, **g))
    frames = _frames(DTYPES[dt], nframes, H, W, seed=100 + nframes)
    kw = dict(rowwisenormalize=rwn, donotnormalize=dnn, movavgn=mov)
    assert all(rec.get_reference(r) is None for r in (BACKGROUND, PI, DARK))
    held = {}
    for role, fr in ((BACKGROUND, frames), (DARK, frames[::-1]), (PI, frames[-1:])):
        got = _capture(rec, role, fr, device, pad, offset)
        want = capture_model.capture(role, fr, **kw)
        _same(got, want, "role %d" % role)
        held[role] = want
        _same(rec.get_reference(role), want, "fdoct_get_reference, role %d" % role)   # out_host is what the handle holds
    got = _capture(rec, NONE, frames, device, pad, offset)
    _same(got, capture_model.capture(NONE, frames, **kw), "FDOCT_REF_NONE")
    for role, want in held.items():                                                     # ... and NONE changed no role
        _same(rec.get_reference(role), want, "role %d after FDOCT_REF_NONE" % role)
    rec.close()


@pytest.mark.parametrize("mov", [0, 3])
@pytest.mark.parametrize("pad,offset", [(5, 1), (5, 0), (0, 1), (0, 0), (8, 0)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_alignment_of_device_frames_selects_the_path(dt, pad, offset, mov):
    """Device-resident frames are read where they lie, so their pointer and pitch decide between the 16-byte loads and the
    sample-by-sample loop (host frames are repacked on upload and never do): a pointer one sample past a 16-byte boundary, a
    pitch that is not a multiple of 16 bytes, each alone and together, next to the aligned cases (W = 200: 16-byte aligned rows
    for every type, with a scalar tail for u8; pad 8 keeps the pitch a multiple of 16 for u16 / f32 / f64)."""
    g = GEOM["odd"]
    W, H = g["width"], g["height"]
    kw = dict(rowwisenormalize=0, donotnormalize=1, movavgn=mov)
    rec = Reconstructor(Config(**g, **kw))
    frames = _frames(DTYPES[dt], 5, H, W, seed=200 + pad + offset)
    for role, fr in ((BACKGROUND, frames), (PI, frames[2:3])):
        d = _DeviceFrames(fr, pad, offset)
        assert (d.ptr % 16 == 0) == (offset == 0)
        got = rec.capture_reference_device(role, d.ptr, d.dtype, d.n, d.pitch, out=True)
        _same(got, capture_model.capture(role, fr, **kw), "role %d" % role)
    rec.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("mediann,binx,biny,dt", [(3, 2, 2, "u8"), (5, 2, 2, "u16"), (3, 1, 2, "u16"), (5, 3, 3, "u8"),
                                                   (0, 2, 2, "u16"), (3, 1, 1, "u8"), (5, 1, 2, "u8"), (3, 3, 3, "u16")])
def test_capture_behind_the_front_end(mediann, binx, biny, dt, device):
    W, H = 128, 96
    kw = dict(rowwisenormalize=1, donotnormalize=0, movavgn=2) if binx == 2 else dict(rowwisenormalize=0, donotnormalize=1, movavgn=0)
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=1024, numdisplaypoints=512, **kw))
    rec.set_frontend(mediann, binx, biny)
    raw = _frames(DTYPES[dt], 3, H * biny, W * binx, seed=7)
    fe = dict(mediann=mediann, binx=binx, biny=biny)
    _same(_capture(rec, BACKGROUND, raw, device), capture_model.capture(BACKGROUND, raw, **kw, **fe), "background")
    _same(_capture(rec, PI, raw[1:2], device, pad=3), capture_model.capture(PI, raw[1:2], **kw, **fe), "pi, padded raw rows")
    _same(rec.get_reference(BACKGROUND), capture_model.capture(BACKGROUND, raw, **kw, **fe))
    wlo, whi = capture_model.frame_minmax(raw, **fe)
    if device:   # device frames, device results
        import torch
        d = _DeviceFrames(raw, pad=3)
        res = torch.zeros(2 * d.n, dtype=torch.float64, device="cuda")
        rec.frame_minmax_device(d.ptr, d.dtype, d.n, d.pitch, res.data_ptr(), res.data_ptr() + 8 * d.n)
        rec.synchronize()
        lo, hi = res[:d.n].cpu().numpy(), res[d.n:].cpu().numpy()
    else:
        lo, hi = rec.frame_minmax(raw)
    _same(lo, wlo)
    _same(hi, whi)
    rec.close()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_sim_variant_takes_the_frame_itself(dt):
    W, H = 128, 96
    kw = dict(rowwisenormalize=1, donotnormalize=0, movavgn=3)
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=1024, numdisplaypoints=512, variant=VARIANT_SIM, **kw))
    frames = _frames(DTYPES[dt], 3, H, W, seed=9)
    if dt in ("f32", "f64"):
        frames[0, 0, 0] = -0.0                      # a copy keeps the sign of zero; a sum from 0.0 would not
    for role in (BACKGROUND, PI):
        got = _capture(rec, role, frames[:1], device=(role == PI))
        _same(got, frames[0].astype(np.float64), "sim, role %d" % role)
        with pytest.raises(FdoctError) as e:
            rec.capture_reference(role, frames)     # nframes must be 1 (sim:803-825)
        assert e.value.code == -1 and "one frame" in str(e.value)
        _same(rec.get_reference(role), frames[0].astype(np.float64))
    for role in (DARK, NONE):                       # rule 2 with the config's flags, no moving average in the sim variant
        _same(_capture(rec, role, frames, device=True), capture_model.capture(role, frames, sim=True, **kw), "sim, role %d" % role)
    rec.close()


def test_argument_errors_leave_the_previous_frame_in_place():
    W, H = 128, 96
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=1024, numdisplaypoints=512))
    frames = _frames(np.uint16, 2, H, W, seed=3)
    before = {BACKGROUND: rec.capture_reference(BACKGROUND, frames, out=True), PI: rec.capture_reference(PI, frames[:1], out=True),
              DARK: rec.capture_reference(DARK, frames[1:], out=True)}
    lib, h = rec.lib, rec.h
    out = np.full((H, W), -7.0)
    p = frames.ctypes.data

    def refused(rc, text):
        assert rc == -1, rc
        assert text in lib.fdoct_last_error(h).decode(), lib.fdoct_last_error(h)
        for role, want in before.items():
            _same(rec.get_reference(role), want, "role %d after a refused call" % role)
        assert np.all(out == -7.0)

    refused(lib.fdoct_capture_reference(h, PI, p, capi.DTYPE_U16, capi.MEM_HOST, 2, 0, out.ctypes.data), "one frame")
    refused(lib.fdoct_capture_reference(h, 4, p, capi.DTYPE_U16, capi.MEM_HOST, 1, 0, out.ctypes.data), "bad role")
    refused(lib.fdoct_capture_reference(h, -1, p, capi.DTYPE_U16, capi.MEM_HOST, 1, 0, out.ctypes.data), "bad role")
    refused(lib.fdoct_capture_reference(h, BACKGROUND, p, capi.DTYPE_U16, capi.MEM_HOST, 2, 2 * W - 2, out.ctypes.data), "pitch smaller than a row")
    refused(lib.fdoct_capture_reference(h, BACKGROUND, p, capi.DTYPE_U16, capi.MEM_HOST, 2, 2 * W + 1, out.ctypes.data), "aligned")
    refused(lib.fdoct_capture_reference(h, BACKGROUND, p, capi.DTYPE_U16, capi.MEM_HOST, 0, 0, out.ctypes.data), "bad arguments")
    refused(lib.fdoct_capture_reference(h, BACKGROUND, None, capi.DTYPE_U16, capi.MEM_HOST, 1, 0, out.ctypes.data), "bad arguments")
    refused(lib.fdoct_capture_reference(h, BACKGROUND, p, 9, capi.MEM_HOST, 1, 0, out.ctypes.data), "bad dtype")
    refused(lib.fdoct_capture_reference(h, BACKGROUND, p, capi.DTYPE_U16, 5, 1, 0, out.ctypes.data), "bad arguments")
    refused(lib.fdoct_frame_minmax(h, p, capi.DTYPE_U16, capi.MEM_HOST, 2, 0, None, None, capi.MEM_HOST), "no output")
    refused(lib.fdoct_frame_minmax(h, p, capi.DTYPE_U16, capi.MEM_HOST, 2, 2, out.ctypes.data, None, capi.MEM_HOST), "pitch smaller than a row")
    refused(lib.fdoct_get_reference(h, NONE, out.ctypes.data, out.size, None), "role must be")
    refused(lib.fdoct_get_reference(h, BACKGROUND, out.ctypes.data, out.size - 1, None), "buffer smaller")
    # the front end's own refusals, before anything runs: float frames, and the 7 x 7 median of 16-bit frames
    rec.set_frontend(7, 1, 1)
    refused(lib.fdoct_capture_reference(h, BACKGROUND, p, capi.DTYPE_U16, capi.MEM_HOST, 2, 0, out.ctypes.data), "7x7 median")
    f32 = frames.astype(np.float32)
    assert lib.fdoct_capture_reference(h, BACKGROUND, f32.ctypes.data, capi.DTYPE_F32, capi.MEM_HOST, 2, 0, out.ctypes.data) == -2
    assert "front end" in lib.fdoct_last_error(h).decode()
    for role, want in before.items():
        _same(rec.get_reference(role), want)
    # a setter's frame is what fdoct_get_reference shows, too: one spectrum for all rows, and unset again
    rec.set_frontend(0, 1, 1)
    rec.set_background(np.arange(W, dtype=np.float64))
    _same(rec.get_reference(BACKGROUND), np.arange(W, dtype=np.float64)[None])
    rec.set_dark(None)
    assert rec.get_reference(DARK) is None
    rec.close()


SHAPES = {"fused": (dict(width=2048, height=8, numfftpoints=2048, numdisplaypoints=1024), None),
          "wave": (dict(width=640, height=4, numfftpoints=2560, numdisplaypoints=512, increasefftpointsmultiplier=4), None),
          "generic": (dict(width=200, height=6, numfftpoints=2560, numdisplaypoints=320, increasefftpointsmultiplier=4), -2)}


@pytest.mark.parametrize("with_pi_dark", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_captured_frame_is_the_handles_frame(shape, with_pi_dark):
    """Handle A captures; handle B is handed the model's doubles through the setters.  Their exported states are the same
    bytes and they reconstruct the same frames to the same bits, on every kernel family."""
    g, plan = SHAPES[shape]
    W, H = g["width"], g["height"]
    kw = dict(rowwisenormalize=0, donotnormalize=1, movavgn=0)
    a, b = Reconstructor(Config(**g, **kw)), Reconstructor(Config(**g, **kw))
    rng = np.random.default_rng(5)
    bgf = (synth.make_frames(20, 16, W, H) * rng.uniform(0.7, 1.0, (16, 1, 1))).astype(np.uint16)
    dark = rng.integers(3, 9, (3, H, W)).astype(np.uint16)
    pif = synth.make_frames(40, 1, W, H).astype(np.uint16)
    a.capture_reference(BACKGROUND, bgf)
    b.set_background(capture_model.capture(BACKGROUND, bgf, **kw))
    if with_pi_dark:
        d = _DeviceFrames(dark)
        a.capture_reference_device(DARK, d.ptr, d.dtype, d.n, d.pitch)
        a.capture_reference(PI, pif)
        b.set_dark(capture_model.capture(DARK, dark, **kw))
        b.set_pi_frame(capture_model.capture(PI, pif, **kw))
    for r in (a, b):
        if plan is not None:
            r.set_plan(plan)
    assert a.export_state().tobytes() == b.export_state().tobytes()
    frames = synth.make_frames(3, 2, W, H)
    ba, da = a.process(frames)
    bb, db = b.process(frames)
    assert a.last_kernel() == b.last_kernel()
    if shape == "generic":
        assert a.last_kernel() == capi.KERNEL_GENERIC
    elif not with_pi_dark:   # (the plain set-up: the shape's own family)
        assert a.last_kernel() in ((capi.KERNEL_FUSED,) if shape == "fused" else (capi.KERNEL_WAVE, capi.KERNEL_WAVE_JIT))
    assert np.array_equal(ba.view(np.uint32), bb.view(np.uint32)) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    a.close()
    b.close()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("device_out", [False, True])
def test_frame_minmax_is_exact(dt, device_out):
    import torch
    W, H = 200, 6
    rec = Reconstructor(Config(**GEOM["odd"]))
    frames = _frames(DTYPES[dt], 5, H, W, seed=31)
    top = 255 if dt == "u8" else 60000
    frames[1, H - 1, W - 1] = top         # the extreme is the frame's very last sample ...
    frames[2, H - 1, W - 1] = 0           # ... as a minimum, too (float frames: below anything the noise reaches)
    if dt in ("f32", "f64"):
        frames[2, H - 1, W - 1] = -1e6
    frames[3, 0, 0] = top
    want_lo, want_hi = capture_model.frame_minmax(frames)
    assert want_hi[1] == top and want_lo[2] == frames[2, H - 1, W - 1]
    for pad, offset in ((0, 0), (3, 1)):   # aligned rows (200 samples: a scalar tail for u8) and the unaligned path
        if device_out:
            d = _DeviceFrames(frames, pad, offset)
            res = torch.zeros(2 * d.n, dtype=torch.float64, device="cuda")
            rec.frame_minmax_device(d.ptr, d.dtype, d.n, d.pitch, res.data_ptr(), res.data_ptr() + 8 * d.n)
            rec.synchronize()
            lo, hi = res[:d.n].cpu().numpy(), res[d.n:].cpu().numpy()
        else:
            lo, hi = rec.frame_minmax(_host_view(frames, pad) if pad else frames)
        _same(lo, want_lo, "min, pad %d" % pad)
        _same(hi, want_hi, "max, pad %d" % pad)
    # either result may be left out
    only = np.zeros(5)
    rec._check(rec.lib.fdoct_frame_minmax(rec.h, frames.ctypes.data, capi._NP2DT[frames.dtype], capi.MEM_HOST, 5, 0, None,
                                          only.ctypes.data, capi.MEM_HOST))
    _same(only, want_hi)
    rec.close()


def test_c2_sized_capture_and_minmax_on_device_frames():
    """2048 x 1000 u16, 16 device-resident frames: a frame that fills the chip.  Its 256 000 runs of 8 samples stay below the
    262 144 threads of a 256-CU card's capped grid, so capture_accumulate_kernel's loop body runs once per thread here, and with
    16 frames the min / max fold reads exactly one 64-lane stride of partials.  The second strides are taken by
    tests/test_gpu_stage_grids.py: test_capture_beyond_one_pass_of_the_grid, test_one_large_frame_takes_the_folds_second_stride
    and test_more_frames_than_workgroups."""
    W, H, n = 2048, 1000, 16
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 65536, (n, H, W), dtype=np.uint16)
    d = _DeviceFrames(frames)
    for mov, dnn in ((0, 1), (3, 0)):
        kw = dict(rowwisenormalize=0, donotnormalize=dnn, movavgn=mov)
        rec = Reconstructor(Config(width=W, height=H, numfftpoints=2048, numdisplaypoints=1024, **kw))
        got = rec.capture_reference_device(BACKGROUND, d.ptr, d.dtype, n, d.pitch, out=True)
        _same(got, capture_model.capture(BACKGROUND, frames, **kw), "C2, movavgn %d" % mov)
        _same(rec.get_reference(BACKGROUND), got)
        rec.close()
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=2048, numdisplaypoints=1024))
    import torch
    res = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    rec.frame_minmax_device(d.ptr, d.dtype, n, d.pitch, res.data_ptr(), res.data_ptr() + 8 * n)
    rec.synchronize()
    wlo, whi = capture_model.frame_minmax(frames)
    _same(res[:n].cpu().numpy(), wlo)
    _same(res[n:].cpu().numpy(), whi)
    rec.close()


def test_host_harness_captures_its_background_and_prints_max_intensity(tmp_path):
    """host/bscanfft_sim --capture-background 4 --max-intensity on a written .ocv file: the C++ caller's 'b' key is one call,
    and its B-scans are the Python path's to the bit."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    exe = os.path.join(ROOT, "host", "bscanfft_sim")
    W, H, N, D = 128, 96, 1024, 512
    frames = _frames(np.uint16, 6, H, W, seed=55)
    f_ocv = str(tmp_path / "frames.ocv")
    io.write_ocv(f_ocv, frames.reshape(6 * H, W))
    prefix = str(tmp_path / "out")
    cmd = [exe, "--frames", f_ocv, "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N),
           "--numdisplaypoints", str(D), "--out", prefix, "--capture-background", "4", "--max-intensity"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
    bscan = np.fromfile(prefix + "_bscan.f32", np.float32).reshape(-1, D, H)
    db = np.fromfile(prefix + "_bscandb.f32", np.float32).reshape(-1, D, H)
    assert bscan.shape[0] == 2
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    got = rec.capture_reference(BACKGROUND, frames[:4], out=True)
    _same(got, capture_model.capture(BACKGROUND, frames[:4]))
    pb, pdb = rec.process(frames[4:], layout=capi.LAYOUT_TRANSPOSED)
    rec.close()
    assert np.array_equal(bscan.view(np.uint32), pb.view(np.uint32)) and np.array_equal(db.view(np.uint32), pdb.view(np.uint32))
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Max intensity = ")]
    assert lines == ["Max intensity = %d" % int(frames[4 + i].max()) for i in range(2)]
