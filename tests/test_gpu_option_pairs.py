"""Every kernel family of the reconstruction chain on the covering array of tests/option_pairs.py: per family a couple of dozen
cases in which every pair of levels of two chain options that can be on together is on together at least once -- sample type,
background, pi and dark frame, the normalisations, averages, moving average, dispersion phase, display depth, layout, the images
asked for, one- or two-word division, entry point and alignment, front end, band-pass, launch size, window.  The fixed suites hold
each option to the oracle one at a time per family; a defect in a line that two options share shows only here.

One test per (family, case): the handle is built from the case with the setters in the catalogue's order, the call goes through the
case's entry point, last_kernel() is the kernel the catalogue names (an empty jit_note() where that is a run-time compiled one), and
the images, brought to row-major, are held to helpers.check_mag / check_db against the f32 restatement and to helpers.check_truth
against the chain in double.  An image not asked for is None and the other one is still checked.  Band-pass cases are held to the
chain in double alone, |gpu - truth| <= 0.5 x the tolerance: the library evaluates that stage in double, the restatement in float.
Device-pointer cases hand over result buffers filled with NaN with 8 floats of guard on either side: the guards stay NaN, everything
between is finite.

Per family, the joint most at risk -- row independence across the options: the family's first whole-frame-normalised case with
averages > 1 run again with its two groups of frames swapped gives the two B-scans swapped, bit for bit."""
import os

import numpy as np
import pytest

import helpers
import option_pairs as op
from fdoct_amd import LAYOUT_TRANSPOSED, Reconstructor, capi

pytestmark = pytest.mark.gpu

GUARD = 8                 # floats on either side of a device result buffer
CASES = [pytest.param(name, n, id="%s #%02d %s" % (name, n, op.case_id(c))) for name in op.FAMILY_IDS for n, c in enumerate(op.generate(name))]


@pytest.fixture(scope="module", autouse=True)
def _one_compile_cache(tmp_path_factory):
    """Run-time compiled kernels of the whole module share one cache directory: every option set is compiled once per run."""
    old = os.environ.get("FDOCT_JIT_CACHE")
    os.environ["FDOCT_JIT_CACHE"] = str(tmp_path_factory.mktemp("jit"))
    yield
    if old is None:
        os.environ.pop("FDOCT_JIT_CACHE", None)
    else:
        os.environ["FDOCT_JIT_CACHE"] = old


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _handle(fam, case, i):
    """The handle of a case; the setters in the order of option_pairs.NAMES."""
    r = Reconstructor(i.cfg)
    try:
        if fam.setup == "any-option":
            r.set_plan(-1, True)
        elif fam.setup == "rows-in-hbm":
            r.set_plan(-3)
        r.set_background(i.yb)
        if i.yp is not None:
            r.set_pi_frame(i.yp)
        if i.yd is not None:
            r.set_dark(i.yd)
        if i.phase is not None:
            r.set_dispersion_phase(i.phase)
        if case.division == "one":
            r.set_precise_division(False)
        if i.front is not None:
            r.set_frontend(*i.front)
        if i.bandpass:
            r.set_bandpass(True)
        if case.launch == "grid2":
            r.set_launch(0, 2)
        if i.window is not None:
            r.set_window(i.window)
        if fam.setup == "staged":
            r.set_staged(True)
    except Exception:
        r.close()
        raise
    return r


def _run(fam, case, r, frames, what):
    """(bscan, db) in row-major order, None where not asked for, through the case's entry point and layout."""
    want_b, want_d = case.outputs != "db", case.outputs != "bscan"
    cfg = r.cfg
    H, D, A = cfg.height, cfg.numdisplaypoints, cfg.averages
    G = frames.shape[0] // A
    transposed = case.layout == "DxH"
    lay = LAYOUT_TRANSPOSED if transposed else 0
    if case.entry == "host":
        b, d = r.process(frames, want_db=want_d, want_bscan=want_b, layout=lay)
    else:
        import torch
        off, out_off = op.frames_offset(case), op.OFFGRID_BYTES if case.entry == "offgrid" else 0
        es = frames.dtype.itemsize
        rows, row_bytes = frames.shape[0] * frames.shape[1], frames.shape[2] * es
        pitch = op.device_pitch(fam, case)
        assert pitch >= row_bytes and (pitch - row_bytes < 32) and (case.entry == "device") == (pitch == row_bytes)
        buf = torch.zeros(off + rows * pitch + 64, dtype=torch.uint8, device="cuda")
        src = torch.from_numpy(np.array(frames, order="C").view(np.uint8).reshape(rows, row_bytes)).cuda()
        buf[off:off + rows * pitch].view(rows, pitch)[:, :row_bytes] = src
        assert (buf.data_ptr() + off) % 16 == off
        n = G * H * D
        first = GUARD + out_off // 4      # floats in front of the image: the guard, and (offgrid) one float more
        outs = [torch.full((first + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda") if w else None for w in (want_b, want_d)]
        assert all(o is None or (o.data_ptr() + 4 * first) % 16 == out_off for o in outs)
        dt = {np.dtype(np.uint8): capi.DTYPE_U8, np.dtype(np.uint16): capi.DTYPE_U16, np.dtype(np.float32): capi.DTYPE_F32,
              np.dtype(np.float64): capi.DTYPE_F64}[frames.dtype]
        r.process_device(buf.data_ptr() + off, dt, frames.shape[0], pitch, *[None if o is None else o.data_ptr() + 4 * first for o in outs], lay)
        r.synchronize()
        res = []
        for o, img in zip(outs, ("linear", "dB")):
            if o is None:
                res.append(None)
                continue
            o = o.cpu().numpy()
            assert np.isnan(o[:first]).all() and np.isnan(o[first + n:]).all(), "%s: the %s image's guard floats were written" % (what, img)
            assert np.isfinite(o[first:first + n]).all(), "%s: the %s image holds values that are not finite" % (what, img)
            res.append(o[first:first + n].reshape((G, D, H) if transposed else (G, H, D)))
        b, d = res
    assert (b is None) == (not want_b) and (d is None) == (not want_d), what + ": an image that was not asked for"
    for x in (b, d):
        assert x is None or x.shape == ((G, D, H) if transposed else (G, H, D)), (what, x.shape)
    if transposed:
        b, d = [None if x is None else np.ascontiguousarray(np.transpose(x, (0, 2, 1))) for x in (b, d)]
    want_kernel = op.expected_kernel(fam, case)
    assert r.last_kernel() == want_kernel, "%s: kernel %d, expected %d (%s)" % (what, r.last_kernel(), want_kernel, r.jit_note())
    if want_kernel == capi.KERNEL_WAVE_JIT:
        assert r.jit_note() == "", what + ": " + r.jit_note()
    return b, d


@pytest.mark.parametrize("name,n", CASES)
def test_option_pair_case(name, n):
    fam = op.family(name)
    case = op.generate(name)[n]
    what = "%s, case %d (%s)" % (name, n, op.case_id(case))
    i = op.inputs(name, case)
    mag_o, db_o, mag_t, db_t = op.reference(name, case)
    r = _handle(fam, case, i)
    try:
        b, d = _run(fam, case, r, i.frames, what)
    finally:
        r.close()
    tid = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    if b is not None:
        assert np.isfinite(b).all(), what + ": non-finite output"
        g, o = helpers.truth_ratios(b, mag_t, mag_o)
        helpers.TRUTH_LOG.append((tid, what, g, o))
        print("%s: |gpu - truth| / tol = %.3g (f32 restatement %.3g)" % (what, g, o))
    if d is not None:
        assert np.isfinite(d).all(), what + ": non-finite dB"
    if case.bandpass == "on":
        if b is not None:
            assert g <= helpers.TRUTH_LIMIT, "%s: |gpu - truth| / tol = %.3g under the band-pass" % (what, g)
        if d is not None:
            gd = float(helpers.db_ratio(d, db_t, mag_t).max())
            print("%s: dB %.3g x the bound the tolerance implies" % (what, gd))
            assert gd <= 1.0, "%s: the dB image is %.3g x the bound the tolerance implies from the chain in double" % (what, gd)
        return
    if b is not None:
        helpers.check_truth(b, mag_t, mag_o, what)
        helpers.check_mag(b, mag_o, what)
    if d is not None:
        helpers.check_db(d, db_o, mag_o, what)


@pytest.mark.parametrize("name", op.FAMILY_IDS)
def test_swapped_groups_give_swapped_images(name):
    """Row independence across the options: nothing a kernel keeps per frame or per group -- the whole-frame extremes, the
    averaging sum, the sim variant's choice of frame -- may leak from one group of a call into the other."""
    fam = op.family(name)
    case = op.row_independence_case(name)
    what = "%s (%s)" % (name, op.case_id(case))
    i = op.inputs(name, case)
    A = case.averages
    per_group = i.frames.shape[0] // op.GROUPS
    assert per_group == A
    swapped = np.ascontiguousarray(np.concatenate([i.frames[per_group:], i.frames[:per_group]]))
    r = _handle(fam, case, i)
    try:
        b0, d0 = _run(fam, case, r, i.frames, what)
        b1, d1 = _run(fam, case, r, swapped, what + ", groups swapped")
    finally:
        r.close()
    for x0, x1, img in ((b0, b1, "linear"), (d0, d1, "dB")):
        if x0 is None:
            continue
        assert not np.array_equal(_bits(x0[0]), _bits(x0[1])), what + ": the two groups give the same image"
        bad = np.argwhere(_bits(x1) != _bits(x0[::-1]))
        assert bad.size == 0, "%s: %d values of the %s image differ once the groups are swapped, first at %s" % (what, len(bad), img, bad[0])
