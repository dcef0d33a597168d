"""GPU tests of manual averaging (include/fdoct_manualavg.h) against tests/manualavg_model.py.
  linear output  bit for bit (uint32): the double sums in image order, the IEEE division by m and the one rounding to float are
                 all determined
  dB output      at most one float ulp from the model: the device's double log and NumPy's may differ in their last double
                 bits, and two doubles that close round to equal or adjacent floats.  The share of elements that differ at
                 all is printed (on an MI355X with ROCm 7: none of the 9.0e6 elements these tests compare).
  partial sums   bit for bit (uint64)
plus what is exact: every door (host, device, mixed memory), the 16-byte and the element-wise path, reruns, every split of a
sequence of images into calls; packed slots behind sentinels; refusals that touch nothing.
The launch: 256 threads per workgroup, four floats per lane on the 16-byte path (one on the other), a grid capped at
resident_blocks(CUs, 16 waves per CU, 256) workgroups (fdoct_manualavg.hip)."""
import os
import subprocess

import numpy as np
import pytest

import manualavg_model as m
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64            # floats in front of and behind every device output
SENTINEL = -7777.0
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
REF, KEEP = capi.MANUALAVG_REFERENCE, capi.MANUALAVG_KEEP_ALL
COUNTS = [1, 3, 4, 5, 1023, 1024, 1028 + 1, 96 * 512]
AVERAGES = [1, 2, 3, 5]
DIFF = {"elements": 0, "differ": 0}   # dB elements compared against the model in this session, and those not bit-equal


def _rec():
    return Reconstructor(Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128))


def _nbscans(avg):
    return sorted({1, avg, avg + 1, 2 * (avg + 1) + 1, 17})


_IMAGES = {}


def _images(n, count, seed=0):
    """uniform(1e-5, 50) floats with a few exact repeats from image to image and a few denormal-sized values."""
    key = (n, count, seed)
    if key not in _IMAGES:
        rng = np.random.default_rng(1000 * seed + count % 997 + n)
        a = rng.uniform(1e-5, 50.0, (n, count)).astype(np.float32)
        for k in range(1, n):
            idx = rng.integers(0, count, 3)
            a[k, idx] = a[k - 1, idx]
        a[rng.integers(0, n, 4), rng.integers(0, count, 4)] = np.float32(1e-40)
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]


def _ordered(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _check(mean, db, want_mean, want_db, what):
    """The linear image bit for bit, the dB within one ulp; returns the share of dB elements that differ at all."""
    assert mean.shape == want_mean.shape and db.shape == want_db.shape, what
    assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32)), what + ": linear output differs from the model"
    d = np.abs(_ordered(db) - _ordered(want_db))
    DIFF["elements"] += d.size
    DIFF["differ"] += int((d > 0).sum())
    assert d.size == 0 or d.max() <= 1, "%s: dB %d ulp from the model" % (what, d.max())
    return float((d > 0).mean()) if d.size else 0.0


def _feed(rec, imgs, splits, mem=DEVICE, out_mem=DEVICE, offset=0, want=(True, True), spare=1):
    """The images over calls of `splits` images each -> (mean, db, emitted per call), concatenated over the calls.  Device outputs
    hold `spare` slots more than the plan says between guard floats; those and the guards must keep the sentinel."""
    import torch
    n, count = imgs.shape
    avg, _, mode, acc = rec.manualavg_state()
    means, dbs, per_call, k = [], [], [], 0
    for s in splits:
        part = np.ascontiguousarray(imgs[k:k + s])
        k += s
        e, acc_after = capi.manualavg_plan(avg, mode, acc, s)
        cap = e + spare
        if mem == DEVICE:
            t = torch.zeros(offset + part.size, dtype=torch.float32, device="cuda")
            t[offset:] = torch.from_numpy(part.ravel().copy()).cuda()
            src = t.data_ptr() + 4 * offset
        else:
            src = part.ctypes.data
        if out_mem == DEVICE:
            outs = [torch.full((2 * GUARD + offset + cap * count,), SENTINEL, dtype=torch.float32, device="cuda") if w else None for w in want]
            ptrs = [None if o is None else o.data_ptr() + 4 * (GUARD + offset) for o in outs]
        else:
            outs = [np.full(2 * GUARD + cap * count, SENTINEL, np.float32) if w else None for w in want]
            ptrs = [None if o is None else o.ctypes.data + 4 * GUARD for o in outs]
        if e == 0 and spare == 0:
            ptrs = [None, None]
        torch.cuda.synchronize()
        import ctypes as C
        got = C.c_int(-1)
        rec._check(rec.lib.fdoct_manualavg_add(rec.h, src, mem, s, ptrs[0], ptrs[1], out_mem, cap, C.byref(got)))
        rec.synchronize()
        assert got.value == e, (got.value, e)
        acc = rec.manualavg_state()[3]
        assert acc == acc_after
        res = []
        for o in outs:
            if o is None:
                res.append(np.zeros((e, count), np.float32))
                continue
            h = o.cpu().numpy() if out_mem == DEVICE else o
            lead = GUARD + (offset if out_mem == DEVICE else 0)
            body = h[lead:lead + cap * count].reshape(cap, count)
            assert (h[:lead] == SENTINEL).all() and (h[lead + cap * count:] == SENTINEL).all(), "guard floats written"
            assert (body[e:] == SENTINEL).all(), "a slot past `emitted` was written"
            res.append(body[:e].copy())
        if mem == DEVICE:
            assert np.array_equal(t.cpu().numpy()[offset:].view(np.uint32), part.ravel().view(np.uint32)), "the input was written"
        means.append(res[0]), dbs.append(res[1]), per_call.append(e)
    return np.concatenate(means), np.concatenate(dbs), per_call


def _model(avg, count, mode, imgs):
    ref = m.ManualAvg(avg, count, mode)
    mean, db = ref.add(imgs)
    return ref, mean, db


@pytest.mark.parametrize("mode", [REF, KEEP])
@pytest.mark.parametrize("count", COUNTS)
def test_parity_with_the_model_on_both_paths(count, mode):
    """Every m and nbscans of the lists, one call each, from aligned device memory (16-byte path where count % 4 == 0 or the
    call has one image; the count % 4 tail with one image) and from pointers one float off (element-wise path)."""
    rec = _rec()
    worst = 0.0
    for avg in AVERAGES:
        for n in _nbscans(avg):
            imgs = _images(n, count)
            ref, want_mean, want_db = _model(avg, count, mode, imgs)
            what = "count %d m %d mode %d nbscans %d" % (count, avg, mode, n)
            for offset in (0, 1):
                rec.manualavg_begin(avg, count, mode)
                mean, db, per_call = _feed(rec, imgs, [n], offset=offset)
                assert per_call == [want_mean.shape[0]] == [m.plan(avg, mode, 0, n)[0]]
                worst = max(worst, _check(mean, db, want_mean, want_db, what + " offset %d" % offset))
                got = rec.manualavg_state(partial=True)
                assert got[:4] == (avg, count, mode, ref.accumulated), what
                assert np.array_equal(got[4].view(np.uint64), ref.acc.view(np.uint64)), what + ": partial sums differ from the model"
    rec.close()
    print("count %d mode %d: dB differs from the model on at most %.4f %% of a call's elements (session: %d of %d)" %
          (count, mode, 100 * worst, DIFF["differ"], DIFF["elements"]))


@pytest.mark.parametrize("mode", [REF, KEEP])
def test_a_count_the_capped_grid_takes_in_two_strides(mode):
    """One and a half strides of the 16-byte path's capped grid, plus four floats: the second stride is a partial one.  From a
    pointer one float off the same elements are six strides of the element-wise path."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stride = cus * (16 // (256 // 64)) * 256 * 4        # resident_blocks(CUs, 16, 256) workgroups x 256 lanes x 4 floats
    count = stride + stride // 2 + 4
    imgs = _images(4, count, seed=2)
    ref, want_mean, want_db = _model(2, count, mode, imgs)
    rec = _rec()
    for offset in (0, 1):
        rec.manualavg_begin(2, count, mode)
        mean, db, _ = _feed(rec, imgs, [4], offset=offset)
        share = _check(mean, db, want_mean, want_db, "count %d offset %d" % (count, offset))
        sums = rec.manualavg_state(partial=True)[4]
        assert np.array_equal(sums.view(np.uint64), ref.acc.view(np.uint64))
    # one image, count % 4 == 1: the 16-byte path with its tail, second stride included
    one = _images(1, count + 1, seed=3)
    ref1, want_mean1, want_db1 = _model(1, count + 1, KEEP, one)
    rec.manualavg_begin(1, count + 1, KEEP)
    mean1, db1, _ = _feed(rec, one, [1])
    _check(mean1, db1, want_mean1, want_db1, "count %d, one image" % (count + 1))
    rec.close()
    print("count %d (%d CUs): dB differs from the model on %.4f %% of the elements" % (count, cus, 100 * share))


@pytest.mark.parametrize("count", [1024, 1029])
@pytest.mark.parametrize("mode", [REF, KEEP])
def test_same_bits_from_every_door_path_rerun_and_split(mode, count):
    imgs = _images(17, count, seed=1)
    _, want_mean, want_db = _model(3, count, mode, imgs)
    rec = _rec()

    def run(splits, **kw):
        rec.manualavg_begin(3, count, mode)
        mean, db, _ = _feed(rec, imgs, splits, **kw)
        sums = rec.manualavg_state(partial=True)
        return mean.view(np.uint32), db.view(np.uint32), sums[3], sums[4].view(np.uint64)

    base = run([17])
    _check(base[0].view(np.float32), base[1].view(np.float32), want_mean, want_db, "count %d mode %d" % (count, mode))

    def same(got, what):
        for a, b in zip(got, base):
            assert np.array_equal(a, b), what

    same(run([17]), "second run")
    same(run([17], offset=1), "element-wise path")
    same(run([17], mem=HOST, out_mem=HOST), "host memory")
    same(run([17], mem=HOST, out_mem=DEVICE), "host in, device out")
    same(run([17], mem=DEVICE, out_mem=HOST), "device in, host out")
    same(run([1] * 17), "17 calls of one image")
    same(run([1] * 17, mem=HOST, out_mem=HOST), "17 calls of one image, host memory")
    for k in range(1, 17):
        same(run([k, 17 - k]), "split %d + %d" % (k, 17 - k))
    same(run([5, 1, 4, 7], spare=0), "four calls, no spare slot, NULL outputs on the calls that emit nothing")
    # the Python form: stacked over the emitted images, in the images' shape
    rec.manualavg_begin(3, count, mode)
    mean, db = rec.manualavg_add(imgs[:9].reshape(9, 1, count))
    mean2, db2 = rec.manualavg_add(imgs[9:])
    assert mean.shape[1:] == (1, count) and mean2.shape[1:] == (count,)
    assert np.array_equal(np.concatenate([mean.reshape(-1, count), mean2]).view(np.uint32), base[0])
    assert np.array_equal(np.concatenate([db.reshape(-1, count), db2]).view(np.uint32), base[1])
    only_mean = rec.manualavg_add(imgs, want_db=False)
    assert only_mean[1] is None and only_mean[0].shape[0] == capi.manualavg_plan(3, mode, base[2], 17)[0]
    rec.close()


def test_a_mean_of_zero_gives_minus_infinity():
    rec = _rec()
    rec.manualavg_begin(2, 8, KEEP)
    imgs = np.zeros((2, 8), np.float32)
    imgs[:, 1] = 2.303
    mean, db = rec.manualavg_add(imgs)
    assert mean.shape == (1, 8) and mean[0, 0] == 0.0 and db[0, 0] == -np.inf and np.isneginf(db[0, [0, 2, 3, 4, 5, 6, 7]]).all()
    _, want_mean, want_db = _model(2, 8, KEEP, imgs)
    _check(mean, db, want_mean, want_db, "zeros")
    rec.close()


def test_refusals_touch_nothing():
    import ctypes as C
    import torch
    count = 1024
    rec = _rec()
    imgs = _images(4, count, seed=5)
    src = torch.from_numpy(imgs.copy()).cuda()
    out = torch.full((2, 4 * count), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = C.c_int(-9)

    def add(bscans=None, mem=DEVICE, n=3, mean=out[0].data_ptr(), db=out[1].data_ptr(), out_mem=DEVICE, cap=4):
        return rec.lib.fdoct_manualavg_add(rec.h, src.data_ptr() if bscans is None else bscans, mem, n, mean, db, out_mem, cap, C.byref(got))

    assert add() == -5 and b"fdoct_manualavg_begin" in rec.lib.fdoct_last_error(rec.h)        # before begin
    with pytest.raises(FdoctError) as e:
        rec.manualavg_state()
    assert e.value.code == -5
    rec.manualavg_begin(2, count)
    assert rec.manualavg_add_device(src.data_ptr(), 1, None, None, 0) == 0        # a call that emits nothing needs no output
    before = rec.manualavg_state(partial=True)
    assert before[3] == 1
    # three more images: b1 is added, b2 emits, b3 is added -- one slot
    assert capi.manualavg_plan(2, REF, 1, 3) == (1, 1)
    assert add(cap=0) == -1 and b"out_capacity" in rec.lib.fdoct_last_error(rec.h)      # one short
    assert add(mean=None, db=None) == -1                                                   # both outputs NULL on an emitting call
    assert add(mean=src.data_ptr()) == -1 and b"overlap" in rec.lib.fdoct_last_error(rec.h)
    assert add(db=src.data_ptr() + 4 * (3 * count - 1)) == -1                              # the input's last float
    assert add(db=out[0].data_ptr() + 4) == -1                                             # the outputs on each other
    assert add(n=0) == -1 and add(n=-1) == -1
    assert add(mem=2) == -1 and add(out_mem=-1) == -1 and add(bscans=0) == -1 and add(cap=-1) == -1
    rec.synchronize()
    after = rec.manualavg_state(partial=True)
    assert after[:4] == before[:4] and np.array_equal(after[4].view(np.uint64), before[4].view(np.uint64))
    assert (out.cpu().numpy() == SENTINEL).all() and np.array_equal(src.cpu().numpy(), imgs) and got.value == -9
    assert add() == 0 and got.value == 1                                                   # and the same call in order goes through
    rec.synchronize()
    _, want_mean, _ = _model(2, count, REF, np.concatenate([imgs[:1], imgs[:3]]))
    assert np.array_equal(out[0].cpu().numpy()[:count].view(np.uint32), want_mean[0].view(np.uint32))
    rec.manualavg_end()
    rec.manualavg_end()                                                                     # without an accumulator: nothing to do
    assert add() == -5                                                                      # after end
    rec.close()


def test_begin_replaces_clone_starts_without_and_close_is_safe():
    rec = _rec()
    rec.manualavg_begin(3, 100)
    rec.manualavg_add(_images(2, 100))
    rec.manualavg_begin(2, 60, KEEP)                        # a second begin replaces the first
    state = rec.manualavg_state(partial=True)
    assert state[:4] == (2, 60, KEEP, 0) and not state[4].any()
    twin = rec.clone_to_device(0)
    with pytest.raises(FdoctError) as e:
        twin.manualavg_state()
    assert e.value.code == -5
    twin.close()
    rec.manualavg_add(_images(1, 60))
    rec.close()                                             # with an accumulator open and work enqueued


def test_process_manualavg_display_on_device_memory():
    """fdoct_process_async (D x H layout) -> fdoct_manualavg_add on the B-scans where they lie -> fdoct_display on the emitted
    dB, one synchronise at the end.  The grey image equals fdoct_display of the model's dB for every emitted image whose dB
    equals the model's bit for bit; the share of dB elements that do is printed, counted as in the parity tests."""
    import torch
    W, H, N, D = 128, 96, 1024, 512
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, averages=1))
    rec.set_background(synth.make_background(W))
    frames = synth.make_frames(0, 7, W, H)
    bscan_host, _ = rec.process(frames, want_db=False, layout=capi.LAYOUT_TRANSPOSED)
    _, want_mean, want_db = _model(2, D * H, REF, bscan_host.reshape(7, -1))
    d_frames = torch.from_numpy(frames.view(np.int16)).cuda()
    d_bscan = torch.empty((7, D, H), dtype=torch.float32, device="cuda")
    d_mean, d_db = torch.empty((2, D, H), dtype=torch.float32, device="cuda"), torch.empty((2, D, H), dtype=torch.float32, device="cuda")
    d_gray = torch.empty((2, D, H), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rec.manualavg_begin(2, D * H)
    rec.process_device(d_frames.data_ptr(), capi.DTYPE_U16, 7, 0, d_bscan.data_ptr(), None, capi.LAYOUT_TRANSPOSED)
    assert rec.manualavg_add_device(d_bscan.data_ptr(), 7, d_mean.data_ptr(), d_db.data_ptr(), 2) == 2
    rec.display_device(d_db.data_ptr(), 2, D, H, d_gray.data_ptr())
    rec.synchronize()
    assert np.array_equal(d_bscan.cpu().numpy(), bscan_host)
    db, gray = d_db.cpu().numpy(), d_gray.cpu().numpy()
    share = _check(d_mean.cpu().numpy().reshape(2, -1), db.reshape(2, -1), want_mean, want_db, "end to end")
    assert np.array_equal(gray, rec.display(db))
    model_gray = rec.display(want_db.reshape(2, D, H))
    equal_images = 0
    for g in range(2):
        if np.array_equal(db[g].view(np.uint32).ravel(), want_db[g].view(np.uint32)):
            equal_images += 1
            assert np.array_equal(gray[g], model_gray[g])
    print("end to end: dB bit-equal to the model on %.4f %% of the elements, %d of 2 images entirely" % (100 * (1 - share), equal_images))
    assert rec.manualavg_state()[3] == 1
    rec.close()


def test_host_harness_writes_the_emitted_images_like_the_python_path(tmp_path):
    """host/bscanfft_sim --manual-averages 2 on 7 frames writes exactly two images, equal to the Python path's bit for bit;
    --manual-keep-all writes three."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    W, H, N, D = 128, 96, 1024, 512
    frames = synth.make_frames(0, 7, W, H)
    yb = synth.make_background(W)
    (tmp_path / "f.bin").write_bytes(frames.tobytes())
    (tmp_path / "b.bin").write_bytes(yb.tobytes())
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(yb)
    bscan, _ = rec.process(frames, want_db=False, layout=capi.LAYOUT_TRANSPOSED)
    for flags, mode, emitted in [((), REF, 2), (("--manual-keep-all",), KEEP, 3)]:
        prefix = str(tmp_path / ("out%d" % mode))
        cmd = [os.path.join(ROOT, "host", "bscanfft_sim"), "--frames", str(tmp_path / "f.bin"), "--background", str(tmp_path / "b.bin"),
               "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N), "--numdisplaypoints", str(D),
               "--out", prefix, "--manual-averages", "2", *flags]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-2000:]
        rec.manualavg_begin(2, D * H, mode)
        mean, db = rec.manualavg_add(bscan)
        assert mean.shape == (emitted, D, H)
        got_mean, got_db = np.fromfile(prefix + "_bscanman.f32", np.float32), np.fromfile(prefix + "_bscanman_db.f32", np.float32)
        assert got_mean.size == got_db.size == emitted * D * H
        assert np.array_equal(got_mean.view(np.uint32), mean.ravel().view(np.uint32))
        assert np.array_equal(got_db.view(np.uint32), db.ravel().view(np.uint32))
        assert np.array_equal(np.fromfile(prefix + "_bscan.f32", np.float32).reshape(7, D, H), bscan)   # the B-scans themselves are as before
    bad = subprocess.run(cmd[:-3] + ["--manual-averages", "0"], capture_output=True, text=True, timeout=240)
    assert bad.returncode != 0
    rec.close()
