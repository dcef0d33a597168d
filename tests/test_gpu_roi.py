"""GPU tests of the B-scan readouts (include/fdoct_roi.h) against tests/roi_model.py, the numpy restatement of
printMinMaxAscan / printAvgROI / printPeakHoldAscan: holds and A-scan extremes bit for bit, ROI means and the vibration
readout to 1e-12, the reference's quirks, and the physics end to end -- J0-scaled fringes through the chain on the device,
held on the same stream without a host sync, recover the vibration amplitude of every ROI column."""
import numpy as np
import pytest

import roi_model
from fdoct_amd import Config, FdoctError, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED


def _rec(**kw):
    return Reconstructor(Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128, **kw))


def _in_layout(pics, layout):
    return np.ascontiguousarray(pics if layout == TR else np.transpose(pics, (0, 2, 1)))


def _pictures(n, D, H, seed, loc=20.0, scale=30.0):
    return (loc + scale * np.random.default_rng(seed).standard_normal((n, D, H))).astype(np.float32)


def _hold(rec, slot, pics, layout, device, offset=0):
    """Folds pictures (n, D, H) into a slot from host memory or from a device tensor (offset: floats in front of the image,
    which leaves a device pointer that is not 16-byte aligned)."""
    import torch
    n, D, H = pics.shape
    a = _in_layout(pics, layout)
    if not device:
        rec.peakhold(slot, a, layout)
        return
    t = torch.zeros(offset + a.size, dtype=torch.float32, device="cuda")
    t[offset:] = torch.from_numpy(a.ravel()).cuda()
    torch.cuda.synchronize()
    rec.peakhold_device(slot, t.data_ptr() + 4 * offset, n, D, H, layout)
    rec.synchronize()


def _check_slot(rec, model, slot):
    cols, amax, count = rec.peakhold_values(slot)
    np.testing.assert_array_equal(cols, model.cols[slot - 1].astype(np.float32))
    assert amax == np.float32(model.scalar[slot - 1]) and count == model.count[slot - 1]


def _rois(D, H):
    return [(H // 2, D // 2, 1, 1, 0),                    # 1 x 1
            (0, 0, H, D, H - 1),                         # the whole image
            (0, D - 3, min(3, H), 3, H - 1),             # bottom-left corner
            (H - 2, 0, 2, 2, 0),                         # top-right corner
            (1, 1, max(1, H - 2), D - 2, H // 2),        # one pixel in from every border
            (0, 1, max(1, H // 3), D - 2, H - 1)]        # ascanat outside the ROI's columns


_C2 = {}


def _c2_pictures():
    if "p" not in _C2:
        _C2["p"] = _pictures(32, 1024, 1000, 11)
    return _C2["p"]


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("shape", ["c2", "odd", "single"])
def test_holds_are_bit_exact(shape, device, layout):
    pics = {"c2": _c2_pictures, "odd": lambda: _pictures(5, 33, 7, 12), "single": lambda: _pictures(1, 64, 48, 13)}[shape]()
    n, D, H = pics.shape
    rec = _rec()
    model = roi_model.PeakHold()
    for roi in _rois(D, H):
        rec.set_peakhold_roi(*roi)
        model.set_roi(*roi)
        for s in (1, 2):
            rec.clear_peakhold(s)
            model.clear(s)
        _hold(rec, 1, pics, layout, device)
        model.fold(1, pics)
        _check_slot(rec, model, 1)
        # several calls fold to what one call over the concatenation holds
        k = max(1, n // 3)
        _hold(rec, 2, pics[:k], layout, device)
        _hold(rec, 2, pics[k:], layout, device) if k < n else None
        model.fold(2, pics)
        _check_slot(rec, model, 2)
    if device:  # an image that is not 16-byte aligned (the element-wise loads)
        roi = (1, 2, H - 1, D - 3, 0)
        rec.set_peakhold_roi(*roi)
        model.set_roi(*roi)
        rec.clear_peakhold(3)
        model.clear(3)
        _hold(rec, 3, pics, layout, True, offset=1)
        model.fold(3, pics)
        _check_slot(rec, model, 3)
    rec.close()


def test_hold_quirks():
    rec = _rec()
    model = roi_model.PeakHold()
    pics = _pictures(4, 40, 24, 21)
    neg = -np.abs(_pictures(3, 40, 24, 22)) - 1.0
    # no ROI yet: FDOCT_ERR_STATE (the reference's "ROI (0,0) = not selected" made explicit)
    with pytest.raises(FdoctError) as e:
        rec.peakhold(1, _in_layout(pics, ROW), ROW)
    assert e.value.code == -5
    roi = (3, 5, 10, 20, 1)
    rec.set_peakhold_roi(*roi)
    model.set_roi(*roi)
    # every B-scan below 0 dB: the holds stay at 0 (Mat::zeros, max1val = 0)
    rec.peakhold(4, _in_layout(neg, ROW), ROW)
    model.fold(4, neg)
    cols, amax, count = rec.peakhold_values(4)
    assert (cols == 0).all() and amax == 0 and count == 3
    _check_slot(rec, model, 4)
    for s in (1, 2, 3):
        rec.peakhold(s, _in_layout(pics[s - 1:s + 1], TR), TR)
        model.fold(s, pics[s - 1:s + 1])
    # clearing one slot leaves the others
    rec.clear_peakhold(2)
    model.clear(2)
    for s in (1, 2, 3, 4):
        _check_slot(rec, model, s)
    # setting an ROI resets the column holds of all slots and keeps the scalar holds and counts
    roi2 = (0, 4, 7, 9, 23)
    rec.set_peakhold_roi(*roi2)
    model.set_roi(*roi2)
    for s in (1, 2, 3, 4):
        _check_slot(rec, model, s)
        assert (rec.peakhold_values(s)[0] == 0).all()
    assert rec.peakhold_values(1)[1] > 0
    # invalid ROI (outside the image at hold time, or malformed), slot or ascanat: FDOCT_ERR_INVALID
    for bad in [lambda: rec.set_peakhold_roi(-1, 0, 1, 1, 0), lambda: rec.set_peakhold_roi(0, 0, 0, 1, 0),
                lambda: rec.set_peakhold_roi(0, 0, 1, 0, 0), lambda: rec.peakhold(0, _in_layout(pics, ROW), ROW),
                lambda: rec.peakhold(5, _in_layout(pics, ROW), ROW), lambda: rec.clear_peakhold(0),
                lambda: rec.peakhold_values(5), lambda: rec.vibration(2)]:
        with pytest.raises(FdoctError) as e:
            bad()
        assert e.value.code == -1
    for roi_bad in [(20, 0, 5, 4, 0), (0, 38, 2, 3, 0), (0, 0, 2, 2, 24)]:
        rec.set_peakhold_roi(*roi_bad)
        with pytest.raises(FdoctError) as e:
            rec.peakhold(1, _in_layout(pics, ROW), ROW)
        assert e.value.code == -1
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
def test_ascan_minmax_is_bit_exact_with_the_four_row_mask(layout):
    rec = _rec()
    for n, D, H in [(6, 1024, 100), (5, 33, 7), (3, 5, 4), (2, 8, 3)]:
        pics = _pictures(n, D, H, 31 + D)
        pics[:, 0:4, :] += np.where(np.arange(n) % 2 == 0, 500.0, -500.0)[:, None, None]   # extremes in rows 0-3 must not count
        for ascanat in (0, H // 2, H - 1):
            lo, hi = rec.ascan_minmax(_in_layout(pics, layout), ascanat, layout)
            mlo, mhi = roi_model.min_max_ascan(pics, ascanat)
            np.testing.assert_array_equal(lo, mlo)
            np.testing.assert_array_equal(hi, mhi)
            assert (np.abs(hi) < 400).all() and (np.abs(lo) < 400).all()
    for bad in [dict(D=4, H=6, ascanat=0), dict(D=3, H=6, ascanat=0), dict(D=8, H=6, ascanat=6), dict(D=8, H=6, ascanat=-1)]:
        with pytest.raises(FdoctError) as e:
            rec.ascan_minmax(_in_layout(_pictures(2, bad["D"], bad["H"], 1), layout), bad["ascanat"], layout)
        assert e.value.code == -1
    rec.close()


@pytest.mark.parametrize("layout", [ROW, TR])
def test_roi_mean_against_numpy_in_double(layout):
    import torch
    rec = _rec()
    pics = _pictures(9, 1024, 1000, 41)
    a = _in_layout(pics, layout)
    for ascanat, vertpos, width in [(0, 0, 1), (500, 10, 10), (1, 1021, 998), (0, 512, 999), (990, 3, 9)]:
        got = rec.roi_mean(a, ascanat, vertpos, width, layout)
        want = roi_model.avg_roi(pics, ascanat, vertpos, width)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(rec.roi_mean(a, ascanat, vertpos, width, layout), got)   # bitwise reproducible
    # device pointers, enqueued
    t = torch.from_numpy(a).cuda()
    out = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rec.roi_mean_device(t.data_ptr(), 9, 1024, 1000, 500, 10, 10, out.data_ptr(), layout)
    rec.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), rec.roi_mean(a, 500, 10, 10, layout))
    # the reference's strict guard: ascanat + width == ascans is refused (BscanFFT.cpp:107); the 3 rows must fit
    assert roi_model.avg_roi(pics, 990, 0, 10) is None
    for ascanat, vertpos, width in [(990, 0, 10), (0, 0, 1000), (0, 1022, 5), (-1, 0, 2), (0, 0, 0)]:
        with pytest.raises(FdoctError) as e:
            rec.roi_mean(a, ascanat, vertpos, width, layout)
        assert e.value.code == -1
    rec.close()


def test_vibration_modes_against_the_model():
    rec = _rec(lambdamin=830e-9, lambdamax=871e-9)
    model = roi_model.PeakHold()
    roi = (2, 3, 30, 12, 40)
    rec.set_peakhold_roi(*roi)
    model.set_roi(*roi)
    base = _pictures(2, 24, 48, 51, loc=45.0, scale=2.0)
    rng = np.random.default_rng(52)
    for slot, drop in [(1, 0.0), (2, 0.3), (3, 12.0), (4, 5.0)]:
        p = (base - drop * rng.uniform(0, 2, base.shape)).astype(np.float32)
        rec.peakhold(slot, _in_layout(p, ROW), ROW)
        model.fold(slot, p)
    lam = (830e-9 + 871e-9) / 2
    for mode in (3, 4):
        for lambda0 in (None, 1310e-9):
            prof, disp, err = rec.vibration(mode, lambda0)
            mprof, mdisp, merr = model.vibration(mode, lam if lambda0 is None else lambda0)
            np.testing.assert_allclose(prof, mprof, rtol=1e-12, atol=1e-12)
            assert abs(disp - mdisp) <= 1e-12 * abs(mdisp) + 1e-15
            if mode == 3:
                assert abs(err - merr) <= 1e-12 * abs(merr) + 1e-15
            else:
                assert np.isnan(err)
    assert len(set(np.round(model.cols[0] - model.cols[2], 3))) > 5   # the differences spread over the table
    rec.close()


def _vibrating_frames(W, H, amps, z_um, seed):
    """weak_fringe_frame's reflector with one fringe amplitude per A-scan (row): I = S (1 + a_r cos(4 pi n z / lambda)),
    0.9 full scale, u16 with the camera's quantisation as the only noise."""
    lam = synth.lambdas(W)
    S = synth.source_spectrum(W)
    fringe = np.asarray(amps)[:, None] * np.cos(4 * np.pi * synth.NS * (z_um * 1e-6) / lam[None, :])
    rng = np.random.default_rng(seed)
    I = S[None, :] * (1.0 + fringe)
    return np.clip(np.rint(I * 0.9 * 65535.0 + rng.uniform(-0.5, 0.5, I.shape)), 0, 65535).astype(np.uint16)


@pytest.mark.parametrize("layout", [ROW, TR])
@pytest.mark.parametrize("geometry", ["c2", "shipped_ini"])
def test_vibration_amplitude_end_to_end_through_the_chain(geometry, layout):
    """Slots 1 and 2: a static reflector; slot 3: the same fringe scaled by J0(x_j), x_j = 0.2 .. 2.2 across the ROI's
    A-scans (the time average of a fringe vibrating with amplitude A_j, x_j = 4 pi A_j / lambda0).  The chain runs on device
    frames, the holds read its device dB output on the same stream with no host sync in between, and mode 3 recovers every
    x_j to within one step of the reference's table."""
    import torch
    from scipy.special import j0
    if geometry == "c2":
        W, H, N, D, M, x0 = 2048, 1000, 2048, 1024, 1, 300
    else:   # build/BscanFFT.ini's acquisition shape: W 640, numfftpoints 2560, zero-pad x4, 320 display points
        W, H, N, D, M, x0 = 640, 64, 2560, 320, 4, 10
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    rec = Reconstructor(cfg)
    rec.set_background(synth.make_background(W))
    w, amp, z_um = 41, 0.02, 150.0
    xs = 0.2 + 0.05 * np.arange(w)
    static = np.full(H, amp)
    vib = static.copy()
    vib[x0:x0 + w] = amp * j0(xs)
    frames = {1: [_vibrating_frames(W, H, static, z_um, s) for s in (1, 2)],
              2: [_vibrating_frames(W, H, static, z_um, s) for s in (3, 4)],
              3: [_vibrating_frames(W, H, vib, z_um, s) for s in (5, 6)]}
    # the reflector's depth bin, from one static frame (set-up only)
    _, db0 = rec.process(frames[1][0])
    b0 = int(np.argmax(db0[0, x0, 8:])) + 8
    assert 12 <= b0 < D - 12
    rec.set_peakhold_roi(x0, b0 - 6, w, 12, x0 + w // 2)
    shape = (2, D, H) if layout == TR else (2, H, D)
    dev_frames = {s: torch.from_numpy(np.stack(f).view(np.int16)).cuda() for s, f in frames.items()}
    dbs = {s: torch.empty(shape, dtype=torch.float32, device="cuda") for s in frames}
    torch.cuda.synchronize()
    for s in (1, 2, 3):
        rec.process_device(dev_frames[s].data_ptr(), capi.DTYPE_U16, 2, 0, 0, dbs[s].data_ptr(), layout)
        rec.peakhold_device(s, dbs[s].data_ptr(), 2, D, H, layout)
    kernel = rec.last_kernel()
    prof, disp, err = rec.vibration(3)
    lam0 = float(np.float32((cfg.lambdamin + cfg.lambdamax) / 2))
    x_rec = prof * 4 * roi_model.PI / (lam0 * 1e9)
    assert np.abs(x_rec - xs).max() <= 0.05 + 1e-9, np.c_[xs, x_rec]
    # the holds are those of the chain's own output
    model = roi_model.PeakHold()
    model.set_roi(x0, b0 - 6, w, 12, x0 + w // 2)
    for s in (1, 2, 3):
        model.fold(s, roi_model.picture(dbs[s].cpu().numpy(), layout))
        _check_slot(rec, model, s)
    if geometry == "shipped_ini":
        assert kernel in (capi.KERNEL_WAVE, capi.KERNEL_WAVE_JIT), kernel
    rec.close()


def test_holds_on_a_user_stream_interleaved_with_the_chain():
    """fdoct_set_stream to a caller's stream: process_async and peakhold calls interleaved on it hold exactly what the
    chain wrote (read back afterwards), i.e. each hold ran after the call that wrote its input."""
    import torch
    W, H, N, D = 2048, 200, 2048, 1024
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(synth.make_background(W))
    roi = (20, 30, 150, 200, 5)
    rec.set_peakhold_roi(*roi)
    model = roi_model.PeakHold()
    model.set_roi(*roi)
    st = torch.cuda.Stream()
    frames = [torch.from_numpy(synth.make_frames(4 * i, 4, W, H).view(np.int16)).cuda() for i in range(4)]
    dbs = [torch.full((4, H, D), -1000.0, dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    rec.set_stream(st.cuda_stream)
    for i in range(4):
        rec.process_device(frames[i].data_ptr(), capi.DTYPE_U16, 4, 0, 0, dbs[i].data_ptr(), ROW)
        rec.peakhold_device(1 + i % 2, dbs[i].data_ptr(), 4, D, H, ROW)
    cols1, amax1, n1 = rec.peakhold_values(1)
    st.synchronize()
    for i in range(4):
        model.fold(1 + i % 2, roi_model.picture(dbs[i].cpu().numpy(), ROW))
    _check_slot(rec, model, 1)
    _check_slot(rec, model, 2)
    assert n1 == 8 and amax1 > 0
    rec.set_stream(None)
    rec.close()


def test_host_harness_prints_the_roi_report(tmp_path):
    """host/bscanfft_sim --roi-mean ascanat,vertpos,width: one "Mean of ROI at .. = .. dB" line per output B-scan (the
    reference's ROIreport text, BscanFFT.cpp:116), the mean of the dB image it wrote."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "host"), "-s"])
    W, H, N, D = 128, 96, 1024, 512
    frames = synth.make_frames(0, 3, W, H)
    (tmp_path / "f.bin").write_bytes(frames.tobytes())
    (tmp_path / "b.bin").write_bytes(synth.make_background(W).tobytes())
    prefix = str(tmp_path / "out")
    cmd = [os.path.join(root, "host", "bscanfft_sim"), "--frames", str(tmp_path / "f.bin"), "--background", str(tmp_path / "b.bin"),
           "--width", str(W), "--height", str(H), "--bits", "16", "--numfftpoints", str(N), "--numdisplaypoints", str(D),
           "--out", prefix, "--roi-mean", "40,10,20"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Mean of ROI at 40 = ")]
    db = np.fromfile(prefix + "_bscandb.f32", np.float32).reshape(-1, D, H)
    want = roi_model.avg_roi(db, 40, 10, 20)
    assert len(lines) == 3
    got = np.array([float(ln.split("=")[1].split()[0]) for ln in lines])
    np.testing.assert_allclose(got, want, rtol=0, atol=6e-7)
    bad = subprocess.run(cmd[:-1] + ["76,10,20"], capture_output=True, text=True, timeout=240)   # 76 + 20 == H: refused
    assert bad.returncode != 0 and "fdoct_roi_mean" in bad.stderr
