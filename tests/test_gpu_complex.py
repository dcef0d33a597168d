"""GPU tests of the complex A-scan (include/fdoct_complex.h, Reconstructor.process_complex): both kernel families that write it,
held to tests/complex_model.py -- parity with the oracle's float composition within the project's tolerance on complex moduli, and
the adjudication against the composition in double -- with the family asserted in every case.

Wave route (the wave-per-row kernel compiled at run time with FDOCT_WAVE_OPT_CXOUT): a zero-padded shape, C2's power-of-two shape
(which fdoct_process gives to the fused kernel), a row displayed beyond numfftpoints / 2 (the mirror and bin N/2), complex rows
(C3's phase), and pi + dark frames under the sim variant's whole-frame normalise (the min / max pre-pass).  Generic route
(generic_kernel's CX form): Bluestein at half length, the full-length zero-pad stage, 512 and 1024 threads, the one-buffer form,
an odd numfftpoints (the full complex transform), doubles with non-integer samples (the split pre-pass), the front end's 2 x 2
binning, and every wave shape again with run-time compilation off.  Then what holds for both: the modulus is what fdoct_process
writes as raw magnitudes on the same family; the D x H layout is the row-major one transposed, bit for bit, with partial tiles both
ways; device memory gives what host memory gives; a batch of more rows than one pass of the launch's grid equals the base batch
it repeats, bit for bit; the refusals leave a poisoned output alone; a fused handle still runs the fused kernel afterwards, with
the same bits.

Cases are 2 frames of 12 rows unless they say otherwise.  The worst ratios of every comparison go to helpers.TRUTH_LOG (the suite's
truth table) and, when FDOCT_COMPLEX_TABLE names a file, into that file (profiles/complex_truth_table.txt is such a run)."""
import os

import numpy as np
import pytest

import chain_grid_sizes as s
import complex_model as cm
import helpers
import oracle_lib as orc
from fdoct_amd import VARIANT_SIM, Config, FdoctError, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
WAVE, GENERIC = capi.KERNEL_WAVE_JIT, capi.KERNEL_GENERIC
H, NF = 12, 2
WAVE_MAX_WAVES = 16   # waves of one workgroup of wave_kernel at most (1024 threads: wave_block_of, fdoct_wave_rules.h)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("FDOCT_COMPLEX_TABLE")
    if path and cm.RATIOS:
        with open(path, "w") as f:
            f.write("# case | |gpu - f32 model| / tol | |gpu - truth| / tol | |f32 model - truth| / tol   (tol = 1e-4 |ref| + 1e-6 rowmax|ref|, complex moduli)\n")
            for what, par, g, o in cm.RATIOS:
                f.write("%-78s %.4f  %.4f  %.4f\n" % (what, par, g, o))


def _handle(cfg, yb, yp=None, yd=None, phase=None, jit=True, generic=False, frontend=None):
    rec = Reconstructor(cfg)
    rec.set_background(yb)
    if yp is not None:
        rec.set_pi_frame(yp)
    if yd is not None:
        rec.set_dark(yd)
    if phase is not None:
        rec.set_dispersion_phase(phase)
    if not jit:
        rec.set_jit(False)
    if generic:
        rec.set_plan(-2)
    if frontend:
        rec.set_frontend(0, *frontend)
    return rec


def _poisoned(shape):
    return np.full(shape, np.complex64(complex(np.nan, -7.0)), np.complex64)


def _complex(rec, frames, layout=ROW):
    n, h, d = frames.shape[0], rec.cfg.height, rec.cfg.numdisplaypoints
    out = _poisoned((n, d, h) if layout == TR else (n, h, d))
    got = rec.process_complex(frames, layout=layout, out=out)
    assert got is out and np.isfinite(out.view(np.float32)).all()
    return out


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.complex64, what
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32), err_msg=what)


# ---- the two routes against the model -----------------------------------------------------------------------------------------------
# (what, family, W, M, N, D, frame type, options)
CASES = [
    ("wave: 200 x4 -> 2560, D 320, u16", WAVE, 200, 4, 2560, 320, np.uint16, ""),
    ("wave: 2048 -> 2048, D 1024 (C2's shape)", WAVE, 2048, 1, 2048, 1024, np.uint16, ""),
    ("wave: 640 -> 640, D 640, u8 (mirror, bin N/2)", WAVE, 640, 1, 640, 640, np.uint8, ""),
    ("wave: 2048 -> 2048, D 1024, C3's phase", WAVE, 2048, 1, 2048, 1024, np.uint16, "phase"),
    ("wave: 200 x4 -> 2560, D 320, pi + dark, sim normalise", WAVE, 200, 4, 2560, 320, np.uint16, "pi dark sim"),
    ("generic: 2048 -> 2002, D 1001 (Bluestein at half length)", GENERIC, 2048, 1, 2002, 1001, np.uint16, ""),
    ("generic: 322 x4 -> 1288, D 320 (Bluestein, full-length zero-pad)", GENERIC, 322, 4, 1288, 320, np.uint16, ""),
    ("generic: 2048 x4 -> 8192, D 1024 (512 threads)", GENERIC, 2048, 4, 8192, 1024, np.uint16, ""),
    ("generic: 2400 x4 -> 9600, D 1000 (1024 threads)", GENERIC, 2400, 4, 9600, 1000, np.uint16, ""),
    ("generic: 64 -> 67, D 67 (odd N: the full complex transform)", GENERIC, 64, 1, 67, 67, np.uint16, ""),
    # GenericPlan::inplace: tests/native/plan_check.expected, "W=4096 M=8 N=32768 D=2048 phase=0 override=-1 ... inplace=1"
    ("generic: 4096 x8 -> 32768, D 2048 (one DFT buffer, in place)", GENERIC, 4096, 8, 32768, 2048, np.uint16, ""),
    ("generic: 100 -> 256, D 100, f64 frames of non-integers (split pre-pass)", GENERIC, 100, 1, 256, 100, np.float64, ""),
    ("generic: 100 -> 256, D 100, 2 x 2 binning of raw u8 frames", GENERIC, 100, 1, 256, 100, np.uint8, "bin2"),
    ("generic: 640 -> 640, D 640, u8, run-time compilation off (mirror)", GENERIC, 640, 1, 640, 640, np.uint8, "nojit"),
    ("generic: 2048 -> 2048, D 1024, C3's phase, run-time compilation off", GENERIC, 2048, 1, 2048, 1024, np.uint16, "phase nojit"),
]


def _setup(W, M, N, D, dt, opts, h=H, nf=NF):
    """(cfg, what process_complex takes, what the model takes, yb, model keywords, handle keywords)"""
    tokens = opts.split()
    ckw = dict(variant=VARIANT_SIM) if "sim" in tokens else {}
    cfg = Config(width=W, height=h, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, **ckw)
    yb = synth.make_background(W).astype(np.float64)
    mkw, hkw = {}, {}
    if "phase" in tokens:
        mkw["phase"] = hkw["phase"] = synth.dispersion_phase(N)
    if "sim" in tokens:
        yb = yb / 65535.0   # (the normalised frame lies in [0, 1])
    rng = np.random.default_rng(31)
    if "pi" in tokens:
        mkw["yp"] = hkw["yp"] = rng.uniform(0.0, 0.02, (h, W))
    if "dark" in tokens:
        mkw["yd"] = hkw["yd"] = rng.uniform(90.0, 110.0, (h, W))
    if "nojit" in tokens:
        hkw["jit"] = False
    if "bin2" in tokens:
        raw = synth.make_frames(4, nf, 2 * W, 2 * h, dtype=np.uint8)
        binned = np.stack([orc.resize_area(f.astype(np.uint16), 2, 2) for f in raw])   # main:958, the oracle's own
        hkw["frontend"] = (2, 2)
        return cfg, raw, binned, yb, mkw, hkw
    if dt == np.float64:
        frames = synth.make_frames(4, nf, W, h).astype(np.float64) / 7.0 + rng.uniform(-0.5, 0.5, (nf, h, W))
        assert not np.any(frames == np.rint(frames))
        return cfg, frames, frames, yb / 7.0, mkw, hkw
    frames = synth.make_frames(4, nf, W, h, dtype=dt)
    return cfg, frames, frames, yb, mkw, hkw


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_both_routes_against_the_model(case):
    what, family, W, M, N, D, dt, opts = case
    cfg, frames, model_frames, yb, mkw, hkw = _setup(W, M, N, D, dt, opts)
    rec = _handle(cfg, yb, **hkw)
    got = _complex(rec, frames)
    fam, note = rec.last_kernel(), rec.jit_note()
    rec.close()
    assert fam == family, "%s: kernel family %d, %s" % (what, fam, note)
    cm.check(got, cfg, model_frames, yb, what, **mkw)


def test_run_time_compilation_off_gives_the_generic_family_and_the_same_values():
    """fdoct_set_jit(h, 0) on 200 x4 -> 2560: the workgroup-per-row kernel runs, and agrees with the wave route as two kernels of
    this library agree (helpers.check_same, on real and imaginary parts: the same arithmetic up to the order of a few roundings)."""
    cfg, frames, _, yb, _, _ = _setup(200, 4, 2560, 320, np.uint16, "")
    out = {}
    for jit in (True, False):
        rec = _handle(cfg, yb, jit=jit)
        out[jit] = _complex(rec, frames)
        assert rec.last_kernel() == (WAVE if jit else GENERIC), rec.jit_note()
        rec.close()
    cm.check(out[False], cfg, frames, yb, "generic: 200 x4 -> 2560, D 320, run-time compilation off")
    rowmax = np.abs(out[True]).max(axis=-1, keepdims=True)
    tol = 0.2 * (helpers.RTOL * np.abs(out[True]) + helpers.ATOL_ROWMAX * rowmax)   # check_same's bound, on the complex difference
    assert (np.abs(out[False].astype(np.complex128) - out[True]) / tol).max() <= 1.0


@pytest.mark.parametrize("family", ["wave", "generic"])
def test_modulus_is_the_magnitude_path_on_the_same_family(family):
    """|X| against fdoct_process with raw magnitudes (no epsilon, averages 1) on the same kernel family: the two differ in the
    last step only, a square root."""
    cfg, frames, _, yb, _, _ = _setup(200, 4, 2560, 320, np.uint16, "")
    generic = family == "generic"
    rec = _handle(cfg, yb, generic=generic)
    rec.set_raw_magnitudes(True)
    mag, _ = rec.process(frames, want_db=False)
    assert rec.last_kernel() == (GENERIC if generic else WAVE), rec.jit_note()
    rec.set_raw_magnitudes(False)
    X = _complex(rec, frames)
    assert rec.last_kernel() == (GENERIC if generic else WAVE), rec.jit_note()
    rec.close()
    helpers.check_same(np.abs(X.astype(np.complex128)), mag, "modulus against raw magnitudes, " + family)


@pytest.mark.parametrize("shape", [(13, 200, 4, 2560, 320, WAVE), (12, 2048, 1, 2002, 1001, GENERIC)], ids=["H 13 x D 320", "H 12 x D 1001"])
def test_transposed_layout_is_the_row_major_one_transposed(shape):
    """Partial 32 x 32 tiles both ways: 13 and 12 rows, 320 = 10 tiles and 1001 = 31 tiles + 9 bins."""
    h, W, M, N, D, family = shape
    cfg, frames, _, yb, _, _ = _setup(W, M, N, D, np.uint16, "", h=h, nf=3)
    rec = _handle(cfg, yb)
    row = _complex(rec, frames, ROW)
    tr = _complex(rec, frames, TR)
    assert rec.last_kernel() == family
    rec.close()
    assert tr.shape == (3, D, h)
    _same_bits(tr, np.transpose(row, (0, 2, 1)), "D x H layout")


def _device_call(rec, frames, layout=ROW, out_off_bytes=0, pad=0):
    """process_complex_device on frames in device memory (rows `pad` bytes apart) into NaN-filled device memory."""
    import torch
    a = np.ascontiguousarray(frames)
    n, rows, w = a.shape
    row = w * a.itemsize
    host = np.zeros((n * rows, row + pad), np.uint8)
    host[:, :row] = a.view(np.uint8).reshape(n * rows, row)
    d_in = torch.from_numpy(host.reshape(-1)).cuda()
    count = n * rec.cfg.height * rec.cfg.numdisplaypoints
    d_out = torch.full((2 * count + 4,), float("nan"), dtype=torch.float32, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    rec.process_complex_device(d_in.data_ptr(), capi._NP2DT[a.dtype], n, row + pad, d_out.data_ptr() + out_off_bytes, layout)
    rec.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("family", ["wave", "generic"])
def test_device_memory_gives_what_host_memory_gives(family):
    W, M, N, D = (200, 4, 2560, 320) if family == "wave" else (2048, 1, 2002, 1001)
    cfg, frames, _, yb, _, _ = _setup(W, M, N, D, np.uint16, "")
    rec = _handle(cfg, yb)
    for layout in (ROW, TR):
        host = _complex(rec, frames, layout)
        flat = _device_call(rec, frames, layout, out_off_bytes=8, pad=8)   # (8-byte aligned, not 16; rows 8 bytes apart)
        assert rec.last_kernel() == (WAVE if family == "wave" else GENERIC)
        assert np.isnan(flat[:2]).all() and np.isnan(flat[2 + 2 * host.size:]).all()   # nothing written outside the result
        _same_bits(flat[2:2 + 2 * host.size].view(np.complex64).reshape(host.shape), host, "device against host memory")
    # an output that is 4-byte but not 8-byte aligned is refused, and nothing is written
    with pytest.raises(FdoctError) as e:
        _device_call(rec, frames, ROW, out_off_bytes=4)
    assert e.value.code == -1 and "8 bytes" in str(e.value)
    out = np.full(2 * NF * H * D + 1, np.float32(-7.0), np.float32)
    lib = rec.lib
    assert lib.fdoct_process_complex(rec.h, frames.ctypes.data, capi.DTYPE_U16, capi.MEM_HOST, NF, 0, out.ctypes.data + 4, capi.MEM_HOST, ROW) == -1
    assert np.all(out == -7.0)
    rec.close()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def wave_tall(rows, cus):
    """More than one pass of the wave-per-row kernel's grid whatever it is: the grid is at most one workgroup per CU and a workgroup
    holds at most WAVE_MAX_WAVES waves, one row each at a time (fdoct_route_value.cpp, wave_launch) -- so one and a half passes of the
    largest launch, and a partial last pass for every number of waves."""
    return 2 * rows >= 3 * WAVE_MAX_WAVES * cus and all(rows % (k * cus) != 0 for k in range(1, WAVE_MAX_WAVES + 1))


@pytest.mark.parametrize("family", ["wave", "generic"])
def test_a_batch_beyond_one_pass_of_the_grid_repeats_its_base_bit_for_bit(family):
    """640 -> 640, D 320, rows of 7: a base batch of 3 frames (21 rows, within one pass: every workgroup or wave takes its first
    row only) and a tall batch whose frame f is the base's frame f mod 3, sized from the CU count.  Rows are independent in both
    kernels (the mean estimate is the row's own), so the tall batch equals the base frame by frame, bit for bit: a row skipped,
    taken twice or stored at another row's address shows exactly."""
    cus = _cus()
    h, base_n = 7, 3
    cfg, base, _, yb, _, _ = _setup(640, 1, 640, 320, np.uint16, "", h=h, nf=base_n)
    if family == "wave":
        n = -(-3 * WAVE_MAX_WAVES * cus // (2 * h))
        while not wave_tall(n * h, cus):
            n += 1
        assert wave_tall(n * h, cus) and base_n * h <= cus
    else:
        n = s.tall_groups(h, cus)
        assert s.generic_tall(n * h, cus) and s.generic_base(base_n * h, cus)
    rec = _handle(cfg, yb, jit=family == "wave")
    want = _complex(rec, base)
    assert rec.last_kernel() == (WAVE if family == "wave" else GENERIC), rec.jit_note()
    cm.check(want, cfg, base, yb, "%s: 640 -> 640, D 320, base batch of %d rows" % (family, base_n * h))
    tall = np.ascontiguousarray(base[np.arange(n) % base_n])
    flat = _device_call(rec, tall)
    assert rec.last_kernel() == (WAVE if family == "wave" else GENERIC)
    rec.close()
    got = flat[:2 * n * h * 320].view(np.complex64).reshape(n, h, 320)
    _same_bits(got, want[np.arange(n) % base_n], "tall batch of %d rows on %d CUs" % (n * h, cus))


def test_refusals_leave_a_poisoned_output_untouched():
    cfg, frames, _, yb, _, _ = _setup(200, 4, 2560, 320, np.uint16, "")

    def refused(rec, fr, code, text):
        out = _poisoned((fr.shape[0], rec.cfg.height, rec.cfg.numdisplaypoints))
        with pytest.raises(FdoctError) as e:
            rec.process_complex(fr, out=out)
        assert e.value.code == code and text in str(e.value), str(e.value)
        v = out.view(np.float32).reshape(-1, 2)
        assert np.isnan(v[:, 0]).all() and np.all(v[:, 1] == -7.0)

    rec = Reconstructor(cfg)
    refused(rec, frames, -5, "background")                      # FDOCT_ERR_STATE
    rec.set_background(yb)
    rec.set_averages(2)
    refused(rec, frames, -2, "averages")                        # FDOCT_ERR_UNSUPPORTED: a complex mean is another quantity
    rec.set_averages(1)
    out = _poisoned((NF, H, 320))
    lib, h = rec.lib, rec.h
    call = lambda fr=frames.ctypes.data, dt=capi.DTYPE_U16, sp=0, n=NF, pitch=0, o=out.ctypes.data, osp=0, lay=ROW: (   # noqa: E731
        lib.fdoct_process_complex(h, fr, dt, sp, n, pitch, o, osp, lay))
    assert call(fr=None) == -1 and call(o=None) == -1 and call(n=0) == -1 and call(n=-3) == -1
    assert call(dt=9) == -1 and call(lay=2) == -1 and call(sp=5) == -1 and call(osp=-1) == -1
    assert call(pitch=2 * 200 - 2) == -1 and b"pitch" in lib.fdoct_last_error(h)
    assert call(o=out.ctypes.data + 4) == -1 and b"8 bytes" in lib.fdoct_last_error(h)
    v = out.view(np.float32).reshape(-1, 2)
    assert np.isnan(v[:, 0]).all() and np.all(v[:, 1] == -7.0)
    assert rec.last_kernel() == capi.KERNEL_NONE
    np.testing.assert_array_equal(_complex(rec, frames), _complex(rec, frames))   # ... and the handle works afterwards
    rec.close()
    # rows only the long-row path takes: 2048 x8 -> 65536 (a 32768-point transform does not fit a compute unit's LDS)
    big = Config(width=2048, height=2, numfftpoints=65536, numdisplaypoints=2048, increasefftpointsmultiplier=8)
    rec = Reconstructor(big)
    rec.set_background(synth.make_background(2048))
    fr = synth.make_frames(0, 1, 2048, 2)
    refused(rec, fr, -2, "long-row")
    mag, _ = rec.process(fr, want_db=False)                     # (fdoct_process takes them, on that path)
    assert rec.last_kernel() == capi.KERNEL_LONG_ROWS and np.isfinite(mag).all()
    rec.close()


def test_a_fused_handle_runs_the_fused_kernel_before_and_after_with_the_same_bits():
    """C2's handle: fdoct_process, the complex call (on the wave-per-row kernel), fdoct_process again.  The complex call reads
    the handle's plan and tables and changes none of them."""
    cfg, frames, _, yb, _, _ = _setup(2048, 1, 2048, 1024, np.uint16, "")
    rec = _handle(cfg, yb)
    before = rec.process(frames)
    assert rec.last_kernel() == capi.KERNEL_FUSED
    X = _complex(rec, frames)
    assert rec.last_kernel() == WAVE, rec.jit_note()
    after = rec.process(frames)
    assert rec.last_kernel() == capi.KERNEL_FUSED
    tr = rec.process(frames, layout=TR)
    assert rec.last_kernel() in (capi.KERNEL_FUSED, capi.KERNEL_FUSED_TRANSPOSED)
    rec.close()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(tr[0], np.transpose(before[0], (0, 2, 1)))
    # and the complex call's modulus is that image without its epsilon, to the rule two kernels of this library are held to
    helpers.check_same(np.abs(X.astype(np.complex128)) + 1e-5, before[0], "modulus against the fused kernel's image")
