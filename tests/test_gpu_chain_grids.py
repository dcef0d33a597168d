"""GPU tests of the reconstruction chain beyond one pass of its grids: generic_kernel's row tickets and the rotation of their
counter words (fdoct_generic.hip, fdoct_route.cpp::launch_family_generic), the passes in front of the chain (f64_split_kernel,
movavg_kernel, movavg_f64_kernel<double> and <float>), the whole-frame min / max pre-pass (minmax_fast_kernel, minmax_kernel,
minmax_finish_kernel and launch_minmax's slices) and the transpose pass (transpose_kernel, transpose64_kernel and
launch_transpose's slices).  The fixed tests of these kernels stay within one pass: a workgroup's first row, one stride of a
loop, one slice of a grid dimension.  The cases here are sized from the card's CU count by tests/chain_grid_sizes.py (held to
their conditions on the CPU by tests/test_chain_grid_sizes.py), and every test asserts the inequality that puts it beyond the
pass -- and its base batch within one -- before it launches anything.

No tolerance of its own.  Rows are independent in the workgroup-per-row kernel (its mean estimate is the row's own middle
sample; rows share nothing but their frame's min / max), so a BASE batch of 3 averaging groups, tens of rows, is held to the
oracle by helpers.check_mag / check_db as they are, and a TALL batch that repeats the base's groups (group g = base group
g mod 3) must equal the base bit for bit, group by group: a row that is skipped, taken twice or addressed wrongly shows exactly,
and the oracle only ever sees the base.  Wherever that identity is asserted the handle is forced to the workgroup-per-row kernel
(set_plan(-2)) and last_kernel() is asserted in both runs -- the fused kernels share a mean estimate between the rows of a wave
and promise no such identity.  Every call goes through process_device on device memory (process() would cut a host batch into
pipeline chunks) into outputs pre-filled with NaN.  The min / max placements are held to the oracle directly.

On an MI355X (256 CUs) the cases are: tall batches of 330 groups x 7 rows = 2310 rows and 461 x 5 = 2305 rows against a base
of 21 and 15 (grid 1536, 512 or 256 workgroups: 1.5, 4.5 or 9 passes, the last one partial); 70 launches of the 2310-row batch
on one handle; 900 000 elements (1.717 passes of 524 288, 160 elements in the last workgroup) against 150 000 in front of the
chain; min / max frames of 35 x 4104 u16 (513 vectors) and 35 x 4112 u8 (257), 3 x 2050 and 3 x 2048; 65 540 frames of 4 x 64 =
262 160 rows (170.7 passes of 1536 tickets, two slices of every sliced grid dimension, 257 workgroups of minmax_finish_kernel).
The module's 36 cases took 5.3 s there run on their own (10.0 s on a card nothing had used yet): 1.8 s (6.7 s) the first case,
the process' first use of the card, 0.5 s each minmax_kernel placement case, 0.4 s the one-buffer form, 0.25 s or less every
other case; 5 min 16 s the whole GPU suite with them.  They add 31 comparisons to the truth
table (the five bases of non-integer doubles take their reference from orc_frame_to_mag, which the table does not see); worst
|gpu - truth| / tol among them 0.188.  Against a library with a bug seeded into each loop named above (a ticket that skips a row,
a plane indexed right only below gridDim.x, a tap one past the row, a stride, slice or partial tile dropped, a counter word left
unzeroed) the cases that cover the loop failed and the others passed."""
import numpy as np
import pytest

import chain_grid_sizes as s
import helpers
import oracle_lib as orc
from fdoct_amd import VARIANT_SIM, Config, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
GENERIC = capi.KERNEL_GENERIC
NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32, "f64": np.float64}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Device:
    """Frames (n, H, W) in device memory: rows `pad` bytes apart, whatever lies between them random (by `seed`)."""

    def __init__(self, frames, pad=0, seed=0):
        import torch
        a = np.ascontiguousarray(frames)
        n, H, W = a.shape
        row = W * a.itemsize
        self.n, self.dtype, self.pitch = n, capi._NP2DT[a.dtype], row + pad
        host = np.random.default_rng([77, seed]).integers(0, 256, (n * H, self.pitch), dtype=np.uint8)
        host[:, :row] = a.view(np.uint8).reshape(n * H, row)
        self.buf = torch.from_numpy(host.reshape(-1)).cuda()
        self.ptr = self.buf.data_ptr()
        assert self.ptr % 16 == 0


def _run(rec, dev, layout=ROW, out_off=0):
    """(linear, dB) of one process_device call into outputs pre-filled with NaN, out_off floats past a 16-byte boundary."""
    import torch
    cfg = rec.cfg
    G, H, D = dev.n // cfg.averages, cfg.height, cfg.numdisplaypoints
    outs = [torch.full((out_off + G * H * D,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    torch.cuda.synchronize()
    rec.process_device(dev.ptr, dev.dtype, dev.n, dev.pitch, outs[0].data_ptr() + 4 * out_off, outs[1].data_ptr() + 4 * out_off, layout)
    rec.synchronize()
    shape = (G, D, H) if layout == TR else (G, H, D)
    return [o[out_off:].cpu().numpy().reshape(shape) for o in outs]


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


def _transposed(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))


def _cycle_frames(base, A, G):
    """G groups of A frames: group g = the base's group g mod 3."""
    b = base.reshape((s.BASE_GROUPS, A) + base.shape[1:])
    return np.ascontiguousarray(b[np.arange(G) % s.BASE_GROUPS]).reshape((G * A,) + base.shape[1:])


def _cycle(out, G):
    return out[np.arange(G) % s.BASE_GROUPS]


def _oracle_doubles(cfg, frames, yb):
    """(linear, dB), both (G, H, D), for frames of non-integer doubles, which the oracle's u16 driver does not take: every
    frame through orc_frame_to_mag (as test_f64_frames_with_non_integer_samples does), then main:1193-1240 on the magnitudes."""
    W, H, N, D, A = cfg.width, cfg.height, cfg.numfftpoints, cfg.numdisplaypoints, cfg.averages
    sim = cfg.variant == VARIANT_SIM
    assert not (sim and A > 1)
    p = orc.make_params(W, H, N, D, cfg.increasefftpointsmultiplier, rowwisenormalize=cfg.rowwisenormalize,
                        donotnormalize=0 if sim else cfg.donotnormalize, movavgn=cfg.movavgn)
    idx, frac = orc.tables(W, cfg.increasefftpointsmultiplier, N, cfg.lambdamin, cfg.lambdamax)
    win = orc.barthann(W)
    mags = np.stack([orc.frame_to_mag(p, f, yb, None, win, idx, frac)[:, :D].astype(np.float64) for f in frames])
    mag = mags.reshape(-1, A, H, D).sum(axis=1) / A + (1e-6 if sim else 1e-5)
    db = 20.0 * np.log(mag) / 2.303
    db[..., 0] = db[..., 1] = db[..., 4]
    return mag, db


def _hold(cfg, frames, yb, mag, db, what, **kw):
    """The base batch against the oracle: the project's rule as it is."""
    assert mag.shape == (frames.shape[0] // cfg.averages, cfg.height, cfg.numdisplaypoints)
    if frames.dtype == np.float64:
        assert not kw and not np.any(frames == np.rint(frames))
        mag_o, db_o = _oracle_doubles(cfg, frames, yb)
    else:
        if frames.dtype == np.float32:                    # camera counts handed over as floats: they embed exactly
            assert np.array_equal(frames, np.rint(frames)) and frames.min() >= 0 and frames.max() <= 65535
            frames = frames.astype(np.uint16)
        mag_o, _, db_t = helpers.oracle_reference(cfg, frames, yb, **kw)
        db_o = np.transpose(db_t, (0, 2, 1))
    helpers.check_mag(mag, mag_o, what)
    helpers.check_db(db, db_o, mag_o, what)


def _handle(cfg, yb, yp=None, yd=None, generic=True):
    rec = Reconstructor(cfg)
    rec.set_background(yb)
    if yp is not None:
        rec.set_pi_frame(yp)
    if yd is not None:
        rec.set_dark(yd)
    if generic:
        rec.set_plan(-2, False)
    return rec


def _identity(cfg, base, yb, G, what, pad=0, sized="rows", **kw):
    """The base batch (3 groups) against the oracle, then the tall one (G groups, cycled) against the base bit for bit.
    Returns (handle, the tall batch on the device, its linear and dB images)."""
    cus, H, A = _cus(), cfg.height, cfg.averages
    assert base.shape[0] == s.BASE_GROUPS * A
    if sized == "rows":
        if not s.generic_base(s.BASE_GROUPS * H, cus):
            pytest.skip("%d CUs: the base batch of %d rows is no single pass" % (cus, s.BASE_GROUPS * H))
        assert s.generic_tall(G * H, cus)
    print("%s: %d CUs, base %d rows, tall %d groups = %d rows" % (what, cus, s.BASE_GROUPS * H, G, G * H))
    rec = _handle(cfg, yb, kw.get("yp"), kw.get("yd"))
    mag0, db0 = _run(rec, _Device(base, pad, seed=1))
    assert rec.last_kernel() == GENERIC, rec.last_kernel()
    _hold(cfg, base, yb, mag0, db0, what + ", base", **kw)
    tall = _Device(_cycle_frames(base, A, G), pad, seed=2)
    mag, db = _run(rec, tall)
    assert rec.last_kernel() == GENERIC, rec.last_kernel()
    _same_bits(mag, _cycle(mag0, G), what + ", tall against base, linear")
    _same_bits(db, _cycle(db0, G), what + ", tall against base, dB")
    return rec, tall, mag, db


# ---- a. row tickets, one case per form of the kernel ---------------------------------------------------------------------------
FORMS = [f[:7] for f in s.GENERIC_FORMS] + [s.GENERIC_ZERO_PAD]


@pytest.mark.parametrize("what,W,M,N,D,A,H", FORMS, ids=[f[0] for f in FORMS])
def test_row_tickets_of_every_kernel_form(what, W, M, N, D, A, H):
    """generic_kernel<256, 6>, <512, 2>, <1024, 1>, <1024, 1, true> and the full-length zero-pad form on a batch of one and a
    half passes of 6 workgroups per CU and a partial last pass: every row past a workgroup's first comes from the ticket
    counter through next_row[parity], and o / H, o - g H, g A + ai address rows far beyond gridDim.x."""
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, averages=A)
    frames = synth.make_frames(17, s.BASE_GROUPS * A, W, H)
    yb = synth.make_background(W).astype(np.float64) + 10.0
    rec, _, _, _ = _identity(cfg, frames, yb, s.tall_groups(H, _cus()), "workgroup-per-row kernel, " + what)
    rec.close()


# ---- b. per-row and per-frame state past the first pass ------------------------------------------------------------------------
OPTIONS = ["2-D background", "2-D dark and pi frames", "row-wise normalisation", "whole-frame normalisation", "u8", "f32", "f64"]


def _small_case(option="plain"):
    """(cfg, base frames, background, oracle keywords) of the small shape under one option."""
    _, W, M, N, D, A, H = s.SMALL[:7]
    rng = np.random.default_rng(5)
    ckw, kw = {}, {}
    frames = synth.make_frames(23, s.BASE_GROUPS * A, W, H)
    yb = synth.make_background(W).astype(np.float64) + 10.0
    if option == "2-D background":
        yb = yb[None, :] * (0.8 + 0.4 * rng.random((H, 1)))
    elif option == "2-D dark and pi frames":
        kw = dict(yp=200.0 * rng.random((H, W)), yd=0.02 * float(frames.max()) * rng.random((H, W)))
    elif option == "row-wise normalisation":
        ckw, yb = dict(rowwisenormalize=1), yb / 65535.0
    elif option == "whole-frame normalisation":       # every frame of the base at a level of its own: (min, max) differ a lot
        ckw, yb = dict(donotnormalize=0), yb / 65535.0
        level = 0.45 + 0.1 * np.arange(frames.shape[0])
        frames = np.rint(frames * level[:, None, None]).astype(np.uint16)
        assert len({(int(f.min()), int(f.max())) for f in frames}) == frames.shape[0]
    elif option == "u8":
        frames = synth.make_frames(23, s.BASE_GROUPS * A, W, H, dtype=np.uint8)
        yb = synth.make_background(W, dtype=np.uint8).astype(np.float64) + 1.0
    elif option == "f32":
        frames = frames.astype(np.float32)
    elif option == "f64":
        frames = frames.astype(np.float64) + rng.uniform(-0.5, 0.5, frames.shape)
    else:
        assert option == "plain"
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, averages=A, **ckw)
    return cfg, frames, yb, kw


@pytest.mark.parametrize("option", OPTIONS)
def test_per_row_and_per_frame_state_past_the_first_pass(option):
    """What a row reads besides its samples, each in turn on the small shape: the H x W background, dark and pi planes at
    r W, the row's own min / max, minmax[g A + ai] of frames far from frame 0, and the 8-bit, float and double loads (the
    doubles through f64_split_kernel, with their low words)."""
    cfg, frames, yb, kw = _small_case(option)
    rec, _, _, _ = _identity(cfg, frames, yb, s.tall_groups(cfg.height, _cus()), "workgroup-per-row kernel, " + option, **kw)
    rec.close()


def test_transposed_layout_of_a_tall_batch():
    """The tall batch in the reference's D x H layout: the chain's row-major images through the transpose pass, bit-identical
    to the row-major result transposed on the host."""
    cfg, frames, yb, _ = _small_case()
    rec, tall, mag, db = _identity(cfg, frames, yb, s.tall_groups(cfg.height, _cus()), "workgroup-per-row kernel, transposed")
    mag_t, db_t = _run(rec, tall, TR)
    assert rec.last_kernel() == GENERIC, rec.last_kernel()
    rec.close()
    _same_bits(mag_t, _transposed(mag), "transposed, linear")
    _same_bits(db_t, _transposed(db), "transposed, dB")


# ---- c. the ticket words' rotation -----------------------------------------------------------------------------------------------
def test_seventy_launches_on_one_handle_without_a_synchronisation():
    """64 counter words, used in turn and zeroed on the stream in front of their launch: 70 launches of the tall batch enqueued
    back to back on one handle reuse six of them while earlier launches may still be running.  Every one of the 70 results
    equals the first, which equals the base."""
    import torch
    cfg, frames, yb, _ = _small_case()
    G = s.tall_groups(cfg.height, _cus())
    n = s.TICKET_LAUNCHES
    assert s.GEN_TICKET_WORDS < n
    rec, tall, mag, db = _identity(cfg, frames, yb, G, "workgroup-per-row kernel, %d launches" % n)
    count = G * cfg.height * cfg.numdisplaypoints
    outs = [torch.full((n, count), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    print("%d launches, %.1f MB of results" % (n, 2 * n * count * 4 / 1e6))
    torch.cuda.synchronize()
    for i in range(n):
        rec.process_device(tall.ptr, tall.dtype, tall.n, tall.pitch, outs[0][i].data_ptr(), outs[1][i].data_ptr(), ROW)
    rec.synchronize()
    assert rec.last_kernel() == GENERIC, rec.last_kernel()
    rec.close()
    for o, first, name in ((outs[0], mag, "linear"), (outs[1], db, "dB")):
        got = o.cpu().numpy().reshape((n,) + first.shape)
        for i in range(n):
            _same_bits(got[i], first, "launch %d of %d, %s" % (i, n, name))


# ---- d. the passes in front of the chain -------------------------------------------------------------------------------------------
# (sample type, bytes between rows, movavgn): what runs in front of the chain
PRE = {
    "u16, moving average": ("u16", 2 * s.PRE_PAD, 2),                  # movavg_kernel
    "u8, moving average": ("u8", s.PRE_PAD, 2),                        # movavg_kernel
    "f32, moving average": ("f32", 4 * s.PRE_PAD, 2),                  # movavg_f64_kernel<float>
    "f32 at an odd pitch, moving average": ("f32", 6, 2),              # movavg_kernel on floats: rows 2 bytes off every other time
    "f64": ("f64", 8 * s.PRE_PAD, 0),                                  # f64_split_kernel
    "f64, moving average": ("f64", 8 * s.PRE_PAD, 2),                  # movavg_f64_kernel<double>
}


def _pre_frames(dt):
    W, H = s.PRE_SHAPE[:2]
    n = s.PRE_BASE_FRAMES
    if dt != "f64":
        return synth.make_frames(40, n, W, H, dtype=np.uint8 if dt == "u8" else np.uint16).astype(NP[dt])
    # doubles none of which is an integer, fringes of 1e-3 of the DC level (test_f64_frames_with_non_integer_samples)
    lam, S = synth.lambdas(W), synth.source_spectrum(W)
    rng = np.random.default_rng(21)
    depth = 40.0 + 6.0 * np.arange(n * H).reshape(n, H, 1)
    fringe = 1e-3 * np.cos(4 * np.pi * synth.NS * (depth * 1e-6) / lam[None, None, :])
    frames = S[None, None, :] * (1.0 + fringe) * 0.9 * 65535.0 / 7.0 + rng.uniform(-0.5, 0.5, (n, H, W))
    assert not np.any(frames == np.rint(frames))
    return frames


@pytest.mark.parametrize("variant", ["main", "sim"])
@pytest.mark.parametrize("kind", list(PRE))
def test_passes_in_front_of_the_chain_beyond_one_pass(kind, variant):
    """2048 x 256 threads stride over rows x W elements.  Base: 150 000 elements, one pass; tall: 900 000, one and a half and a
    last workgroup of 160 elements.  The device frames lie at a pitch wider than the row, and what lies between the rows is
    random and differs between the two batches: a tap or a load that strays there breaks the identity.  sim: the whole-frame
    min / max pre-pass reads the pass's output."""
    dt, pad, mov = PRE[kind]
    W, H, N, D = s.PRE_SHAPE
    base_n, tall_n = s.PRE_BASE_FRAMES, s.PRE_TALL_FRAMES
    assert s.pre_elements(base_n) <= s.PASS and s.beyond(s.pre_elements(tall_n), s.PASS) and s.pre_elements(tall_n) % s.PASS_BLOCK != 0
    pitch = W * np.dtype(NP[dt]).itemsize + pad
    assert pad > 0 and pitch % np.dtype(NP[dt]).itemsize == (2 if "odd" in kind else 0)    # (odd: no multiple of a float's 4 bytes)
    sim = variant == "sim"
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, movavgn=mov, **(dict(variant=VARIANT_SIM) if sim else {}))
    frames = _pre_frames(dt)
    if dt == "f64":
        yb = synth.make_background(W).astype(np.float64) / (65535.0 if sim else 7.0)
    elif sim:
        yb = synth.make_background(W).astype(np.float64) / 65535.0
    else:
        yb = synth.make_background(W, dtype=np.uint8 if dt == "u8" else np.uint16).astype(np.float64) + 1.0
    what = "in front of the chain: %s, %s variant" % (kind, variant)
    print("%s: %d and %d elements, %.3f passes of %d" % (what, s.pre_elements(base_n), s.pre_elements(tall_n), s.pre_elements(tall_n) / s.PASS, s.PASS))
    rec, _, _, _ = _identity(cfg, frames, yb, tall_n, what, pad=pad, sized="elements")
    rec.close()


# ---- e. the min / max pre-pass: where an extreme sits ----------------------------------------------------------------------------
def _extreme_frames(dt, W, H, places, top, body, seed):
    """One frame per placement: the body within `body`, one sample `top` at that placement and one 0 at the next."""
    n = len(places)
    q = synth.make_frames(seed, n, W, H).astype(np.float64) / 65535.0
    f = np.rint(body[0] + q * (body[1] - body[0]))
    assert f.min() >= body[0] and f.max() <= body[1] and top > 1.6 * body[1]     # a missed maximum rescales the frame by more than 1.6
    for k in range(n):
        (r1, c1), (r0, c0) = places[k], places[(k + 1) % n]
        assert r1 != r0
        f[k, r1, c1], f[k, r0, c0] = top, 0
    return f.astype(NP[dt])


def _sim_against_the_oracle(frames, N, D, what, yd=None):
    n, H, W = frames.shape
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, variant=VARIANT_SIM)
    yb = synth.make_background(W).astype(np.float64) / 65535.0
    rec = _handle(cfg, yb, yd=yd, generic=False)
    dev = _Device(frames)
    mag, db = _run(rec, dev)
    rec.close()
    _hold(cfg, frames, yb, mag, db, what, **({} if yd is None else dict(yd=yd)))
    return dev


@pytest.mark.parametrize("dt", ["u16", "u8"])
def test_fast_min_max_kernel_finds_an_extreme_wherever_it_sits(dt):
    """minmax_fast_kernel: 16 workgroups a frame walk its rows r += 16, their threads a row's 16-byte vectors v += 256.  35
    rows of 513 (8-bit: 257) vectors; the five frames of one call carry their 65535 (255) and their 0 at the first sample,
    the last one, in the second vector stride, in the second row round, and in the ragged last round's last stride."""
    H, W, top = s.MINMAX_FAST_H, s.MINMAX_FAST_W[dt], {"u16": 65535, "u8": 255}[dt]
    nv = s.fast_vectors(dt)
    assert nv > s.MINMAX_BLOCK and nv % s.MINMAX_BLOCK == 1 and H > 2 * s.MINMAX_PARTS and H % s.MINMAX_PARTS != 0
    frames = _extreme_frames(dt, W, H, s.fast_places(dt), top, {"u16": (1000, 40000), "u8": (16, 156)}[dt], 60)
    print("minmax_fast_kernel %s: %d frames of %d x %d, %d vectors a row" % (dt, frames.shape[0], H, W, nv))
    dev = _sim_against_the_oracle(frames, 8192, 128, "min / max placements, minmax_fast_kernel, " + dt)
    assert dev.ptr % 16 == 0 and dev.pitch % 16 == 0 and dev.pitch == W * frames.itemsize     # what launch_minmax asks of the fast kernel


@pytest.mark.parametrize("dt", ["u16", "f32"])
def test_min_max_kernel_finds_an_extreme_in_a_later_stride(dt):
    """minmax_kernel: 1024 threads walk a row i += 1024.  Rows of 2050 samples (no whole 16-byte vectors: not the fast
    kernel's), the extremes at the first sample of the second stride and in the ragged third one."""
    W, H = s.MINMAX_SLOW
    assert W > 2 * s.MINMAX_THREADS and W % s.MINMAX_THREADS != 0 and (W * 2) % s.VEC_BYTES != 0
    frames = _extreme_frames(dt, W, H, s.MINMAX_SLOW_AT, 65535, (1000, 40000), 61)
    _sim_against_the_oracle(frames, 4096, 128, "min / max placements, minmax_kernel, " + dt)


def test_min_max_kernel_subtracts_the_dark_frame_first():
    """With an H x W dark frame the extremes are those of x - yd: the largest difference sits at a dip of the dark frame, in
    the second stride, not at the largest sample."""
    W, H = s.MINMAX_DARK
    rng = np.random.default_rng(9)
    q = synth.make_frames(62, 2, W, H).astype(np.float64) / 65535.0
    frames = np.rint(1000 + q * 37000)
    yd = np.rint(rng.uniform(4000, 6000, (H, W)))
    dips, big, low = [(1, s.MINMAX_THREADS), (2, W - 1)], (0, 1500), (0, 1030)     # (all of them past the first stride)
    yd[big], yd[low] = 6000, 6000
    for k, dip in enumerate(dips):
        yd[dip] = 0
        frames[k][dips[k]], frames[k][big], frames[k][low] = 39000, 40000, 0
    frames = frames.astype(np.uint16)
    for k in range(2):
        diff = frames[k].astype(np.float64) - yd
        assert np.unravel_index(diff.argmax(), diff.shape) == dips[k] != np.unravel_index(frames[k].argmax(), diff.shape) == big
        assert np.unravel_index(diff.argmin(), diff.shape) == low and diff.min() == -6000 and diff.max() == 39000
    _sim_against_the_oracle(frames, 2048, 128, "min / max of x - yd, minmax_kernel with a dark frame", yd=yd)


# ---- f. more than 65 535 frames in one launch ---------------------------------------------------------------------------------------
def _many_base():
    W, H = s.MANY_SHAPE[:2]
    q = synth.make_frames(63, s.BASE_GROUPS, W, H).astype(np.float64) / 65535.0
    frames = np.rint(1000 + q * 39000).astype(np.uint16)
    for g, hot in enumerate((50000, 60000, 65535)):      # a frame's scale taken from its neighbour shows
        frames[g, g % H, 7 + g] = hot
    assert [int(f.max()) for f in frames] == [50000, 60000, 65535]
    return frames, synth.make_background(W).astype(np.float64) / 65535.0


@pytest.mark.parametrize("D", [s.MANY_SHAPE[3], s.MANY_D_NARROW])
def test_more_frames_than_one_grid_dimension_holds(D):
    """65 540 frames of 4 x 64 in one call of the sim variant.  Row-major: the second slice of minmax_fast_kernel and its
    partials at partial + f0 16, the 257 workgroups of minmax_finish_kernel, minmax[in_frame] up to 65 539, and 170 passes of
    the ticket; every group equals its base group.  Then the same batch in the D x H layout: two slices of gridDim.z, through
    transpose64_kernel (D = 32) and through transpose_kernel (D = 30), bit-identical to the row-major result transposed on
    the host."""
    W, H, N, _ = s.MANY_SHAPE
    n = s.MANY_FRAMES
    assert n > s.SLICE and -(-n // s.FINISH_BLOCK) > 1 and n % s.FINISH_BLOCK != 0 and (W * 2) % s.VEC_BYTES == 0
    assert s.transpose_wide(H, D) == (D % 4 == 0)
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, variant=VARIANT_SIM)
    frames, yb = _many_base()
    rec, tall, mag, db = _identity(cfg, frames, yb, n, "%d frames, D = %d" % (n, D))
    mag_t, db_t = _run(rec, tall, TR)
    assert rec.last_kernel() == GENERIC != capi.KERNEL_FUSED_TRANSPOSED, rec.last_kernel()
    rec.close()
    _same_bits(mag_t, _transposed(mag), "transposed, linear")
    _same_bits(db_t, _transposed(db), "transposed, dB")


# ---- g. transpose edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D,out_off", s.TRANSPOSE_EDGES)
def test_transpose_pass_at_the_edges_of_its_tiles(H, D, out_off):
    """45 x 67: partial 32-tiles on both sides, nothing a multiple of 4 (transpose_kernel).  68 x 36: a full and a partial
    64-tile of rows, a partial one of columns (transpose64_kernel); the same with the outputs 4 bytes past a 16-byte boundary
    (transpose_kernel).  Three groups, both outputs, bit-identical to the row-major images transposed on the host."""
    W, N = 100, 256
    assert s.transpose_wide(H, D, out_off % 4 == 0) == ((H, D, out_off) == (68, 36, 0))
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D)
    frames = synth.make_frames(29, 3, W, H)
    yb = synth.make_background(W).astype(np.float64) + 10.0
    rec = _handle(cfg, yb)
    dev = _Device(frames)
    mag, db = _run(rec, dev)
    _hold(cfg, frames, yb, mag, db, "transpose edges, %d x %d, row-major" % (H, D))
    mag_t, db_t = _run(rec, dev, TR, out_off)
    assert rec.last_kernel() == GENERIC, rec.last_kernel()
    rec.close()
    _same_bits(mag_t, _transposed(mag), "transposed, linear")
    _same_bits(db_t, _transposed(db), "transposed, dB")
