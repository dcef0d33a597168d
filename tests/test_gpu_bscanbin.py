"""GPU tests of spinjnt's output binning (include/fdoct_bscanbin.h) against tests/bscanbin_model.py on every element:
  linear  tol = 1e-4 |truth| + 1e-6 max over the output A-scan of |truth|;  |gpu - truth| / tol <= max(0.5, |reference-mode - truth| / tol)
  dB      |gpu_db - truth_db| <= 8.686 tol / max(truth - tol, eps) + 2e-4
(bscanbin_model.parity), on real chain outputs of synth frames -- reflector peaks on a floor, where the cubic undershoots --
and on uniform noise; plus what is exact: reruns, the two layouts, the two memory spaces, the clamp at eps, the DC mask."""
import os
import subprocess

import numpy as np
import pytest

import bscanbin_model as m
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64   # floats in front of and behind every device output

# binx, biny, upx, upy: the issue's list ((2, 1) with binvaluey = 2: upx = 2 binx)
FACTORS = [(1, 1, 1, 1), (2, 2, 2, 2), (3, 1, 3, 1), (1, 4, 1, 4), (2, 1, 4, 1), (4, 4, 4, 4), (5, 3, 5, 3), (16, 16, 16, 16)]


def _rec(**kw):
    return Reconstructor(Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128, **kw))


def _in_layout(pics, layout):
    return np.ascontiguousarray(pics if layout == TR else np.transpose(pics, (0, 2, 1)))


def _pictures(a, layout):
    return None if a is None else np.ascontiguousarray(a if layout == TR else np.transpose(a, (0, 2, 1)))


_CHAIN = {}


def _chain_pictures(n, W, H, N, D):
    """Linear B-scans (n, D, H) the chain itself wrote for synth frames."""
    key = (n, W, H, N, D)
    if key not in _CHAIN:
        rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
        rec.set_background(synth.make_background(W))
        bscan, _ = rec.process(synth.make_frames(0, n, W, H), want_db=False, layout=TR)
        rec.close()
        _CHAIN[key] = bscan
    return _CHAIN[key]


def _noise(n, D, H, seed):
    return np.random.default_rng(seed).uniform(0.0, 50.0, (n, D, H)).astype(np.float32)


def _crop(pics, binx, biny):
    n, D, H = pics.shape
    return np.ascontiguousarray(pics[:, :D // biny * biny, :H // binx * binx])


def _run(rec, pics, layout, device, f, mf=None, jscan=None, want=(True, True), offset=0):
    """fdoct_bscan_bin on pictures (n, D, H) from host or device memory -> (linear, dB) pictures (None when not wanted).  The
    device outputs lie between guard floats, which must come back untouched; offset: floats in front of the device input."""
    binx, biny, upx, upy = f
    n, D, H = pics.shape
    a = _in_layout(pics, layout)
    j = None if jscan is None else _in_layout(jscan[None], layout)[0]
    if not device:
        lin, db = rec.bscan_bin(a, binx, biny, upx, upy, mf, jscan=j, layout=layout, want_db=want[1], want_bscan=want[0])
        return _pictures(lin, layout), _pictures(db, layout)
    import torch
    od, oa = capi.bscanbin_size(D, H, binx, biny, upx, upy)
    t = torch.zeros(offset + a.size, dtype=torch.float32, device="cuda")
    t[offset:] = torch.from_numpy(a.ravel()).cuda()
    tj = None if j is None else torch.from_numpy(j).cuda()
    outs = [torch.full((2 * GUARD + n * od * oa,), -7777.0, dtype=torch.float32, device="cuda") if w else None for w in want]
    torch.cuda.synchronize()
    rec.bscan_bin_device(t.data_ptr() + 4 * offset, n, D, H, binx, biny, *[None if o is None else o.data_ptr() + 4 * GUARD for o in outs],
                         upx=upx, upy=upy, multiplyfactor=mf, d_jscan_ptr=None if tj is None else tj.data_ptr(), layout=layout)
    rec.synchronize()
    res = []
    for o in outs:
        if o is None:
            res.append(None)
            continue
        h = o.cpu().numpy()
        assert (h[:GUARD] == -7777.0).all() and (h[-GUARD:] == -7777.0).all(), "guard floats written"
        res.append(_pictures(h[GUARD:-GUARD].reshape((n, od, oa) if layout == TR else (n, oa, od)), layout))
    return res[0], res[1]


def _parity(lin, db, pics, f, what, **kw):
    worst = (0.0, 0.0, 0.0)
    for g in range(pics.shape[0]):
        r = m.parity(None if lin is None else lin[g], None if db is None else db[g], pics[g], f[0], f[1], f[2], f[3],
                     what="%s bin %dx%d up %dx%d B-scan %d" % ((what,) + tuple(f) + (g,)), **kw)
        worst = tuple(max(x, y) for x, y in zip(worst, r))
    return worst


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("f", FACTORS)
def test_c2_chain_images_from_device_memory(f, layout):
    """1000 x 1024 chain outputs (cropped to what the factors divide: 999 A-scans for 3 x 1, 1023 depths for 5 x 3, 992 x 1024
    for 16 x 16 -- sizes that are multiples of neither a tile nor 4 floats)."""
    pics = _crop(_chain_pictures(2, 2048, 1000, 2048, 1024), f[0], f[1])
    rec = _rec()
    lin, db = _run(rec, pics, layout, True, f)
    _, _, under = _parity(lin, db, pics, f, "C2 chain")
    print("C2 chain image, bin %dx%d: truth <= 0 on %.2f %% of the elements" % (f[0], f[1], 100 * under))
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("device", [False, True])
def test_small_chain_images_undershoot_and_noise(device, layout):
    """96 x 512 style images, 5 B-scans per call: chain outputs (the undershoot must occur: truth <= 0 on more than 0.5 % of the
    elements for 2 x 2 and 4 x 4) and uniform noise, every factor set."""
    chain = _chain_pictures(5, 1024, 96, 1024, 512)
    noise = _noise(5, 512, 96, 3)
    rec = _rec()
    for f in FACTORS:
        for name, pics in (("chain", chain), ("noise", noise)):
            p = _crop(pics, f[0], f[1])
            lin, db = _run(rec, p, layout, device, f, mf=f[0] * f[1] * 2)   # binvaluex = 2 in multiplyfactor
            _, _, under = _parity(lin, db, p, f, "96x512 " + name, multiplyfactor=f[0] * f[1] * 2)
            if name == "chain" and f[:2] in ((2, 2), (4, 4)):
                assert under > 0.005, (f, under)
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
def test_tiny_binned_images_and_odd_sizes(layout):
    """Binned sizes of 1 - 3 cells, where the clamp dominates, and sizes that are multiples of nothing; a misaligned device input."""
    rec = _rec()
    cases = [(2, 12, (4, 2, 8, 4)), (6, 4, (2, 3, 2, 3)), (9, 2, (2, 3, 2, 3)), (3, 3, (1, 1, 5, 7)), (16, 16, (16, 16, 64, 64)),
             (33, 7, (1, 1, 1, 1)), (35, 21, (7, 5, 3, 2)), (131, 67, (1, 1, 2, 3)), (26, 39, (13, 13, 1, 1)), (64, 300, (2, 2, 2, 2))]
    for D, H, f in cases:
        pics = _noise(3, D, H, D + H)
        pics[:, D // 2, H // 2] += 4000.0
        for device in (False, True):
            lin, db = _run(rec, pics, layout, device, f)
            _parity(lin, db, pics, f, "%d x %d" % (D, H))
        lin1, db1 = _run(rec, pics, layout, True, f, offset=1)
        np.testing.assert_array_equal(lin1, lin)
        np.testing.assert_array_equal(db1, db)
    rec.close()


def test_exactness_reruns_layouts_memory_spaces_and_output_selection():
    pics = _crop(_chain_pictures(5, 1024, 96, 1024, 512), 3, 2)
    jscan = _noise(1, pics.shape[1], pics.shape[2], 9)[0] * 0.01
    rec = _rec()
    for f, js in [((3, 2, 3, 2), None), ((3, 2, 6, 2), jscan), ((1, 4, 1, 4), None), ((2, 2, 2, 2), jscan)]:
        p = _crop(pics, f[0], f[1])
        j = None if js is None else js[:p.shape[1], :p.shape[2]]
        base = _run(rec, p, TR, True, f, jscan=j)
        for layout in (ROW, TR):
            for device in (False, True):
                got = _run(rec, p, layout, device, f, jscan=j)
                np.testing.assert_array_equal(got[0], base[0])      # reruns, D x H == row-major transposed, host == device
                np.testing.assert_array_equal(got[1], base[1])
                only_lin = _run(rec, p, layout, device, f, jscan=j, want=(True, False))
                only_db = _run(rec, p, layout, device, f, jscan=j, want=(False, True))
                assert only_lin[1] is None and only_db[0] is None
                np.testing.assert_array_equal(only_lin[0], base[0])
                np.testing.assert_array_equal(only_db[1], base[1])
        one = _run(rec, p[:1], TR, True, f, jscan=j)                 # nbscans 1 == the first of 5
        np.testing.assert_array_equal(one[0][0], base[0][0])
        np.testing.assert_array_equal(one[1][0], base[1][0])
        _parity(base[0], base[1], p, f, "exactness", jscan=j)
    rec.close()


def test_dc_mask_jscan_eps_and_the_clamp():
    pics = _chain_pictures(5, 1024, 96, 1024, 512)[:2]
    f = (2, 2, 2, 2)
    floor = {e: np.float32(20.0 * np.log(e) / 2.303) for e in (m.EPS_MAIN, m.EPS_SIM)}
    # dc_mask on: rows 0 and 1 are row 4; truth <= 0 comes out as exactly dB(eps); everything finite
    rec = _rec()
    lin, db = _run(rec, pics, ROW, True, f)
    assert (lin[:, 2:] <= 0).any() and np.isfinite(db).all() and np.isfinite(lin).all()
    np.testing.assert_array_equal(db[:, 0], db[:, 4])
    np.testing.assert_array_equal(db[:, 1], db[:, 4])
    assert (db[:, 2:][lin[:, 2:] <= 0] == floor[m.EPS_MAIN]).all() and db.min() == floor[m.EPS_MAIN]
    # with jscan there is no mask
    j = np.zeros_like(pics[0])
    lin_j, db_j = _run(rec, pics, ROW, True, f, jscan=j)
    assert not np.array_equal(db_j[:, 0], db_j[:, 4])
    _parity(lin_j, db_j, pics, f, "jscan", jscan=j)
    # out_depths <= 4 leaves the rows unmasked
    small = np.ascontiguousarray(pics[:, 100:108])
    for layout in (ROW, TR):
        lin4, db4 = _run(rec, small, layout, True, (1, 2, 1, 1))
        assert db4.shape[1] == 4
        _parity(lin4, db4, small, (1, 2, 1, 1), "out_depths 4")
        lin5, db5 = _run(rec, np.ascontiguousarray(pics[:, 100:105]), layout, True, (2, 1, 2, 1))
        assert db5.shape[1] == 5
        np.testing.assert_array_equal(db5[:, 0], db5[:, 4])
        _parity(lin5, db5, np.ascontiguousarray(pics[:, 100:105]), (2, 1, 2, 1), "out_depths 5")
    rec.close()
    # dc_mask off
    rec = _rec(dc_mask=0)
    for layout in (ROW, TR):
        lin0, db0 = _run(rec, pics, layout, False, f)
        assert not np.array_equal(db0[:, 0], db0[:, 4])
        _parity(lin0, db0, pics, f, "dc_mask off", dc_mask=False)
    rec.close()
    # the sim variant's epsilon
    rec = _rec(variant=capi.VARIANT_SIM)
    lin_s, db_s = _run(rec, pics, TR, True, f)
    assert db_s.min() == floor[m.EPS_SIM] and floor[m.EPS_SIM] < floor[m.EPS_MAIN]
    _parity(lin_s, db_s, pics, f, "sim eps", eps=m.EPS_SIM)
    rec.close()


def test_refusals_leave_the_outputs_untouched():
    import torch
    rec = _rec()
    a = torch.zeros(2 * 64 * 64, dtype=torch.float32, device="cuda")
    out = torch.full((2 * 64 * 64,), 5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for kw, code in [(dict(binx=3), -2), (dict(binx=17), -1), (dict(upx=65), -1), (dict(binx=0), -1)]:
        k = dict(binx=2, biny=2, upx=None)
        k.update(kw)
        with pytest.raises(FdoctError) as e:
            rec.bscan_bin_device(a.data_ptr(), 2, 64, 64, k["binx"], k["biny"], out.data_ptr(), None, upx=k["upx"])
        assert e.value.code == code
    for o, odb in [(a.data_ptr(), None), (a.data_ptr() + 4 * (2 * 64 * 64 - 1), None), (out.data_ptr(), out.data_ptr() + 16), (None, None)]:
        with pytest.raises(FdoctError) as e:
            rec.bscan_bin_device(a.data_ptr(), 2, 64, 64, 2, 2, o, odb)
        assert e.value.code == -1
    rec.synchronize()
    assert (out.cpu().numpy() == 5.0).all() and (a.cpu().numpy() == 0.0).all()
    rec.close()


def test_process_async_bin_display_with_one_synchronise():
    """fdoct_process_async -> fdoct_bscan_bin -> fdoct_display on device memory, one synchronise at the end, equals the
    stepwise result through host memory."""
    import torch
    W, H, N, D = 1024, 96, 1024, 512
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(synth.make_background(W))
    frames = synth.make_frames(0, 3, W, H)
    for layout in (ROW, TR):
        shape = (3, D, H) if layout == TR else (3, H, D)
        bscan_host, _ = rec.process(frames, want_db=False, layout=layout)
        lin_host, db_host = rec.bscan_bin(bscan_host, 2, 2, layout=layout)
        gray_host = rec.display(db_host)
        rec.bscan_bin(bscan_host, 2, 2, upx=4, layout=layout)   # another tap table in between: the next call uploads its own
        d_frames = torch.from_numpy(frames.view(np.int16)).cuda()
        d_bscan = torch.empty(shape, dtype=torch.float32, device="cuda")
        d_lin, d_db = torch.empty_like(d_bscan), torch.empty_like(d_bscan)
        d_gray = torch.empty(shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rec.bscan_bin_device(d_bscan.data_ptr(), 3, D, H, 2, 2, d_lin.data_ptr(), None, layout=layout)   # (uploads the 2 x 2 table)
        rec.process_device(d_frames.data_ptr(), capi.DTYPE_U16, 3, 0, d_bscan.data_ptr(), None, layout)
        rec.bscan_bin_device(d_bscan.data_ptr(), 3, D, H, 2, 2, d_lin.data_ptr(), d_db.data_ptr(), layout=layout)
        rec.display_device(d_db.data_ptr(), 3, shape[1], shape[2], d_gray.data_ptr())
        rec.synchronize()
        np.testing.assert_array_equal(d_lin.cpu().numpy(), lin_host)
        np.testing.assert_array_equal(d_db.cpu().numpy(), db_host)
        np.testing.assert_array_equal(d_gray.cpu().numpy(), gray_host)
    rec.close()


def test_host_harness_applies_the_binning_like_the_python_path(tmp_path):
    """host/bscanfft_sim --bscan-bin 2,2: the .f32 outputs are the binned linear image and its dB, equal to Reconstructor.bscan_bin
    on the chain's output; BX,BY,BINVALUEX,BINVALUEY derives upx, upy and multiplyfactor by the reference's formulas."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    W, H, N, D = 128, 96, 1024, 512
    frames = synth.make_frames(0, 3, W, H)
    yb = synth.make_background(W)
    (tmp_path / "f.bin").write_bytes(frames.tobytes())
    (tmp_path / "b.bin").write_bytes(yb.tobytes())
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(yb)
    bscan, _ = rec.process(frames, want_db=False, layout=TR)
    for spec, (binx, biny, upx, upy, mf) in [("2,2", (2, 2, 2, 2, 4.0)), ("2,1,3,2", (2, 1, 4, 1, 12.0))]:
        prefix = str(tmp_path / ("out" + spec.replace(",", "_")))
        cmd = [os.path.join(ROOT, "host", "bscanfft_sim"), "--frames", str(tmp_path / "f.bin"), "--background", str(tmp_path / "b.bin"),
               "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N), "--numdisplaypoints", str(D),
               "--out", prefix, "--bscan-bin", spec]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-2000:]
        od, oa = capi.bscanbin_size(D, H, binx, biny, upx, upy)
        lin, db = rec.bscan_bin(bscan, binx, biny, upx, upy, mf, layout=TR)
        np.testing.assert_array_equal(np.fromfile(prefix + "_bscan.f32", np.float32).reshape(-1, od, oa), lin)
        np.testing.assert_array_equal(np.fromfile(prefix + "_bscandb.f32", np.float32).reshape(-1, od, oa), db)
    bad = subprocess.run(cmd[:-1] + ["5,1"], capture_output=True, text=True, timeout=240)   # 96 A-scans, binx 5: refused
    assert bad.returncode != 0 and "fdoct_bscan_bin" in bad.stderr
    rec.close()
