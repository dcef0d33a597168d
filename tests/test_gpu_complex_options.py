"""GPU tests of the complex A-scan (include/fdoct_complex.h) on what tests/test_gpu_complex.py leaves out: every chain option,
edge row and table, through both kernel forms that write (re, im) pairs -- the wave-per-row kernel compiled at run time with
FDOCT_WAVE_OPT_CXOUT and generic_kernel's CX form.  Neither form exists in any magnitude instantiation, each has its own untangle
tail (X[b] kept instead of |X[b]|, conjugated above numfftpoints / 2, 8 bytes per bin) and its own early `continue` past the
epilogue; a wrong sign, mirror bin or stale register there leaves the modulus intact, so the magnitude suite cannot see it.  The
cases are tests/complex_cases.py's (held to their conditions on the CPU by tests/test_complex_cases.py), the rule is
tests/complex_model.py's check() and check_rows().

  a. options, one handle each: band-pass, row-wise and whole-frame normalisation, the three smoothmovavg pre-passes, a full-frame
     background, a caller window, f32 frames, the median front end, a colour handle on a channel and on the channel sum -- on
     200 x4 -> 2560 and on 2048 -> 2002 (band-pass: 322 x4 -> 1288) -- and band-pass + row-wise normalisation + pi + dark as one
     option mask of the wave-per-row kernel;
  b. rows with a dispersion phase displayed beyond numfftpoints / 2 (640 -> 640, D 640 and 341), both forms, and the same depths
     without a phase: the mirror;
  c. depths off the 64-bin grid, D = 1, N / 2 + 1 and N, one handle per depth; the bins a shallower run shares with a deeper one
     agree as two kernels of this library agree;
  d. the degenerate frames and planes of tests/degenerate_cases.py: empty rows are 0, cancelled rows within the epsilon rule;
  e. the caller-supplied tables of tests/resample_tables.py on eight families, fdoct_process before and after on the same handle;
  f. a NaN row or a +Inf sample leaves every other row's bits alone, in both layouts;
  g. a staged handle refuses the call and stays staged; the timing read reports 8 bytes per bin.

The kernel family is asserted in every case, on the wave-per-row kernel also that the run-time compiler had nothing to note; the
output starts NaN-poisoned and comes back finite (f. apart).  Frames are 2 x 12 rows, the degenerate and table cases' 1 x 11.
The ratios of every comparison go to helpers.TRUTH_LOG and, when FDOCT_COMPLEX_OPTIONS_TABLE names a file, into that file
(profiles/complex_options_truth_table.txt is such a run)."""
import os

import numpy as np
import pytest

import complex_cases as cc
import complex_model as cm
import degenerate_cases as dg
import helpers
import resample_tables as rt
from fdoct_amd import Config, FdoctError, Reconstructor, build_resample_table, capi, synth

pytestmark = pytest.mark.gpu

ROW, TR = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
FAMILY = {"wave": capi.KERNEL_WAVE_JIT, "generic": capi.KERNEL_GENERIC}


@pytest.fixture(scope="module", autouse=True)
def _table():
    first = len(cm.RATIOS)
    yield
    path = os.environ.get("FDOCT_COMPLEX_OPTIONS_TABLE")
    if path and len(cm.RATIOS) > first:
        with open(path, "w") as f:
            f.write("# case | |gpu - f32 model| / tol | |gpu - truth| / tol | |f32 model - truth| / tol   (tol = 1e-4 |ref| + 1e-6 rowmax|ref|, complex moduli;\n")
            f.write("# rows that are neither empty nor cancelled: tests/complex_model.py, check_rows)\n")
            for what, par, g, o in cm.RATIOS[first:]:
                f.write("%-118s %.4f  %.4f  %.4f\n" % (what, par, g, o))


def _handle(cfg, yb, yp=None, yd=None, phase=None, window=None, bandpass=False, frontend=None, colour=None, jit=True):
    rec = Reconstructor(cfg)
    rec.set_background(yb)
    if yp is not None:
        rec.set_pi_frame(yp)
    if yd is not None:
        rec.set_dark(yd)
    if phase is not None:
        rec.set_dispersion_phase(phase)
    if window is not None:
        rec.set_window(window)
    if bandpass:
        rec.set_bandpass(True)
    if frontend:
        rec.set_frontend(*frontend)
    if colour is not None:
        rec.set_colour_input(colour)
    if not jit:
        rec.set_jit(False)
    return rec


def _poisoned(shape):
    return np.full(shape, np.complex64(complex(np.nan, -7.0)), np.complex64)


def _call(rec, frames, layout=ROW):
    """process_complex into a NaN-poisoned array."""
    n, h, d = np.shape(frames)[0], rec.cfg.height, rec.cfg.numdisplaypoints
    out = _poisoned((n, d, h) if layout == TR else (n, h, d))
    assert rec.process_complex(frames, layout=layout, out=out) is out
    return out


def _complex(rec, frames, layout=ROW):
    out = _call(rec, frames, layout)
    assert np.isfinite(out.view(np.float32)).all()
    return out


def _ran(rec, family, what):
    fam, note = rec.last_kernel(), rec.jit_note()
    assert fam == FAMILY[family], "%s: kernel family %d, %s" % (what, fam, note)
    if family == "wave":
        assert note == "", "%s: %s" % (what, note)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _within_check_same(a, b):
    """Worst |a - b| / (check_same's bound on b), on the complex difference -- it bounds the real and the imaginary part alike: the
    rule tests/test_gpu_complex.py holds two kernels to."""
    tol = 0.2 * (helpers.RTOL * np.abs(b) + helpers.ATOL_ROWMAX * np.abs(b).max(axis=-1, keepdims=True))
    return float((np.abs(a.astype(np.complex128) - b) / np.maximum(tol, 1e-300)).max())


def _run_setup(case, s):
    rec = _handle(s.cfg, s.yb, **s.hkw)
    try:
        got = _complex(rec, s.frames)
        _ran(rec, case.family if isinstance(case, cc.Option) else case.route, case.name)
    finally:
        rec.close()
    return got


# ---- a. options -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.OPTION_CASES, ids=[c.name for c in cc.OPTION_CASES])
def test_every_option_on_both_forms(case):
    s = cc.option_setup(case)
    got = _run_setup(case, s)
    cm.check(got, s.cfg, s.model_frames, s.yb, case.name, **s.mkw)


# ---- b. phase beyond numfftpoints / 2 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.PHASE_CASES, ids=[c.name for c in cc.PHASE_CASES])
def test_rows_displayed_beyond_half_with_and_without_a_phase(case):
    """With a phase the rows are complex: the wave-per-row kernel's CPLX form and generic_kernel's full-length branch, no mirror.
    Without one the bins above N / 2 are the conjugates of their mirror bins; D = 341 ends twenty bins past bin N / 2."""
    s = cc.edge_setup(case)
    got = _run_setup(case, s)
    cm.check(got, s.cfg, s.model_frames, s.yb, case.name, **s.mkw)


# ---- c. depth edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["wave", "generic"])
def test_depths_off_the_64_bin_grid_agree_on_their_shared_bins(route):
    out, failures = {}, []
    cases = [c for c in cc.DEPTH_CASES if c.route == route]
    assert [c.D for c in cases] == list(cc.DEPTHS)
    for case in cases:
        s = cc.edge_setup(case)
        out[case.D] = _run_setup(case, s)
        try:
            cm.check(out[case.D], s.cfg, s.model_frames, s.yb, case.name, **s.mkw)
        except AssertionError as e:
            failures.append(str(e).split("\n")[0])
    for i, lo in enumerate(cc.DEPTHS):
        for hi in cc.DEPTHS[i + 1:]:
            worst = _within_check_same(out[hi][..., :lo], out[lo])
            print("%s: D %d against the first %d bins of D %d: %.3g x check_same's bound" % (route, lo, lo, hi, worst))
            if worst > 1.0:
                failures.append("%s: bins [:%d] of D %d differ from D %d by %.3g x check_same's bound" % (route, lo, hi, lo, worst))
    assert not failures, "\n  ".join(failures)


# ---- d. degenerate rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.DEGENERATE_FAMILIES)
def test_degenerate_frames_and_planes(name):
    family = "wave" if cc.wave_family(name) else "generic"
    failures = []
    for case in cc.DEGENERATE_CASES:
        what = cc.degenerate_name(name, case)
        i = dg.inputs(name, case)
        rec = _handle(i.cfg, i.yb, yp=i.yp, yd=i.yd)
        try:
            got = _complex(rec, i.frames)
            _ran(rec, family, what)
        finally:
            rec.close()
        empty, cancelled = cc.degenerate_rows(case)
        try:
            cm.check_rows(got, i.cfg, i.frames, i.yb, what, empty=empty, cancelled=cancelled, **cc.degenerate_mkw(i))
            if cc.copy_is_exact(case):
                assert np.array_equal(_bits(got[0, dg.COPY]), _bits(got[0, dg.ORDINARY])), what + ": the copy of row 0 differs from row 0"
        except AssertionError as e:
            failures.append(str(e).split("\n")[0])
    assert not failures, "%d of %d cases:\n  " % (len(failures), len(cc.DEGENERATE_CASES)) + "\n  ".join(failures)


# ---- e. caller tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.TABLE_FAMILIES)
def test_every_family_on_custom_tables(name):
    fam = rt.family(name)
    W, M, N, _ = rt.shape(fam)
    i = rt.inputs(name)
    family = "wave" if cc.wave_family(name) else "generic"
    failures = []
    rec = _handle(i.cfg, i.yb, phase=i.phase)
    try:
        for t in cc.tables_of(name):
            what = "%s, table '%s'" % (name, t)
            rec.set_window(rt.window(t, W))        # (None: the built window again)
            if t == "wide":
                rec.set_lambda_range(*rt.WIDE_RANGE)
            else:
                rec.set_resample_table(*rt.family_table(name, t))
            before = rec.process(i.frames)
            got = _complex(rec, i.frames)
            _ran(rec, family, what)
            after = rec.process(i.frames)
            table = rec.get_resample_table()
            try:
                for a, b in zip(before, after):
                    assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b)), what + ": fdoct_process differs after the complex call"
                want = build_resample_table(W, M, N, *rt.WIDE_RANGE) if t == "wide" else rt.family_table(name, t)
                assert np.array_equal(table[0], want[0]) and np.array_equal(table[1].view(np.uint64), want[1].view(np.uint64)), \
                    what + ": fdoct_get_resample_table does not return it"
                cm.check_rows(got, i.cfg, i.frames, i.yb, what, empty=cc.TABLE_EMPTY, cancelled=cc.TABLE_CANCELLED, **cc.table_mkw(name, t))
                assert np.array_equal(_bits(got[0, dg.COPY]), _bits(got[0, dg.ORDINARY])), what + ": the copy of row 0 differs from row 0"
            except AssertionError as e:
                failures.append(str(e).split("\n")[0])
    finally:
        rec.close()
    assert not failures, "%d of %d tables:\n  " % (len(failures), len(cc.tables_of(name))) + "\n  ".join(failures)


# ---- f. row isolation ---------------------------------------------------------------------------------------------------------------
POISONED_ROW = dg.IMPULSE_LEFT       # row 5


@pytest.mark.parametrize("case", cc.ISOLATION_CASES, ids=["plain", "rowwise"])
@pytest.mark.parametrize("name", cc.DEGENERATE_FAMILIES)
def test_a_non_finite_row_leaves_the_other_rows_alone(name, case):
    """The 11-row frame as floats: clean, with row 5 all NaN, and with a single +Inf in row 5.  Every other row of the complex
    output is bit-identical to the clean run, row-major and D x H.  Row 5's own content is not asserted."""
    family = "wave" if cc.wave_family(name) else "generic"
    i = dg.inputs(name, case)
    clean = i.frames.astype(np.float32)
    nan, inf = clean.copy(), clean.copy()
    nan[0, POISONED_ROW] = np.nan
    inf[0, POISONED_ROW, i.frames.shape[2] // 3] = np.inf
    others = [r for r in range(dg.ROWS) if r != POISONED_ROW]
    out = {}
    rec = _handle(i.cfg, i.yb)
    try:
        for what, f in (("clean", clean), ("NaN row", nan), ("+Inf sample", inf)):
            row = _call(rec, f, ROW)
            _ran(rec, family, "%s, %s" % (name, what))
            out[what] = (row, np.transpose(_call(rec, f, TR), (0, 2, 1)))
    finally:
        rec.close()
    row, tr = out["clean"]
    assert np.isfinite(row.view(np.float32)).all()
    _same_bits(np.ascontiguousarray(tr), row, "D x H layout of the clean run")
    empty, cancelled = cc.degenerate_rows(case)
    cm.check_rows(row, i.cfg, i.frames, i.yb, cc.degenerate_name(name, case) + ", f32 frames", empty=empty, cancelled=cancelled)
    for what in ("NaN row", "+Inf sample"):
        for a, c, layout in zip(out[what], out["clean"], ("row-major", "D x H")):
            bad = np.argwhere(_bits(a[0, others]) != _bits(c[0, others]))
            assert bad.size == 0, "%s, %s, %s: %d words of the %s output outside row %d changed, first in row %d" % (
                name, case.opt, what, len(bad), layout, POISONED_ROW, others[bad[0][0]])


# ---- g. small things ---------------------------------------------------------------------------------------------------------------
def test_a_staged_handle_refuses_the_call_and_stays_staged():
    """C2's shape in the two-kernel mode: the complex call needs the workgroup- or wave-per-row kernel, which staged mode has
    none of -- FDOCT_ERR_UNSUPPORTED, the output untouched -- and fdoct_process afterwards is staged still, with the same bits."""
    cfg = Config(width=2048, height=cc.H, numfftpoints=2048, numdisplaypoints=1024)
    frames = synth.make_frames(cc.FIRST_FRAME, cc.NF, 2048, cc.H)
    rec = _handle(cfg, synth.make_background(2048).astype(np.float64))
    try:
        rec.set_staged(True)
        before = rec.process(frames)
        assert rec.last_kernel() == capi.KERNEL_FUSED_STAGED
        out = _poisoned((cc.NF, cc.H, 1024))
        with pytest.raises(FdoctError) as e:
            rec.process_complex(frames, out=out)
        assert e.value.code == -2 and "staged" in str(e.value), str(e.value)
        v = out.view(np.float32).reshape(-1, 2)
        assert np.isnan(v[:, 0]).all() and np.all(v[:, 1] == -7.0)
        after = rec.process(frames)
        assert rec.last_kernel() == capi.KERNEL_FUSED_STAGED
    finally:
        rec.close()
    for a, b in zip(before, after):
        assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("route", ["wave", "generic"])
def test_the_timing_read_reports_eight_bytes_per_bin(route):
    W, M, N, D = cc.WAVE_SHAPE
    cfg = Config(width=W, height=cc.H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M)
    frames = synth.make_frames(cc.FIRST_FRAME, cc.NF, W, cc.H)
    rec = _handle(cfg, synth.make_background(W).astype(np.float64), jit=route == "wave")
    try:
        rec.set_timing(True)
        _complex(rec, frames)
        _ran(rec, route, "timing, " + route)
        t = rec.timing()
    finally:
        rec.close()
    rows = cc.NF * cc.H
    assert t["ascans"] == rows and t["bytes_out"] == rows * D * 8 and t["bytes_in"] == rows * W * 2, t
