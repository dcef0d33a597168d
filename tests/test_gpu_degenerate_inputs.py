"""Every kernel family of the reconstruction chain on the degenerate frames and planes of tests/degenerate_cases.py: rows of
zeros, saturated and constant rows, a row without fringes, single impulses (one of them on a dead background column), a row
alternating between 0 and full scale; backgrounds with dead columns, a column of value 1 and a blocked line; a pi frame equal to
the frame and a dark frame above it; an averaging pair whose second frame is dark; a constant frame and one with its extremes in
its corners under whole-frame normalisation.  The handling of these inputs -- the 0-or-1/(max - min) guard of the normalisations,
x / 0 = 0 in each form the reciprocal background reaches a kernel, the fast paths' mean estimate and two-word division -- is
written out separately in every family; tests/test_degenerate_cases.py holds the oracle to its own conditions on the same cases.

In every case: helpers.check_mag / check_db against the f32 restatement and helpers.check_truth against the chain in double; every
output finite; the rows that hold nothing but zeros before any rounding -- a constant row under row-wise normalisation among them,
its scale is exactly 0 -- equal float32(eps) bit for bit, their dB the dB of that value within one float ulp; with a one-row
background and no whole-frame normalisation the copy of row 0 equals row 0 bit for bit.
The no-fringe row is empty only because a DC level cancels; it is held to the same rule -- a tolerance of about 1e-9.  The kernels that take the second word of 1/background as a half-float pattern
(degenerate_cases.HALF_PATTERN) cannot reach it by design; they are held on the no-fringe row to SURVEY 8(d)'s tolerance with the
peak of the frame's ordinary row 0 in place of the row's own, |gpu - truth| <= 0.5 (1e-4 |truth| + 1e-6 rowmax(truth row 0)), and,
under the rule as it stands, to the row that the half-float pattern gives in double: nothing but that pattern's quantisation may be
left.  No other row gets the wider bound.

Row isolation: f32 frames with row 5 all NaN, or holding one +Inf, leave every other row bit-identical to the clean run (no ticket,
hand-over or loop bound of these kernels depends on sample values; whole-frame normalisation, whose pre-pass spans the frame, is
left out).  Every family takes part but staged mode, which refuses anything but 16-bit samples; float frames reach the D x H
layout through the transpose pass, which every family's run includes."""
import dataclasses
import os

import numpy as np
import pytest

import degenerate_cases as dg
import helpers
from fdoct_amd import Reconstructor, capi

pytestmark = pytest.mark.gpu


def _ordered(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return int(np.abs(_ordered(a) - _ordered(np.broadcast_to(b, np.shape(a)))).max())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Handles:
    """One handle per option set of a family, reused across the cases through its setters."""

    def __init__(self, fam):
        self.fam, self.h = fam, {}

    def get(self, case, i):
        r = self.h.get(case.opt)
        if r is None:
            r = self.h[case.opt] = Reconstructor(dataclasses.replace(i.cfg, averages=1))
            if self.fam.setup == "any-option":
                r.set_plan(-1, True)
        r.set_averages(i.cfg.averages)
        r.set_background(i.yb)
        r.set_pi_frame(i.yp)
        r.set_dark(i.yd)
        return r

    def close(self):
        for r in self.h.values():
            r.close()


def _run(fam, r, frames, want_kernel):
    """(bscan, db) in row-major order, through the family's own route."""
    if fam.setup == "staged":
        r.set_staged(False)
        b0, d0 = r.process(frames)
        assert r.last_kernel() == capi.KERNEL_FUSED
        r.set_staged(True)
    b, d = r.process(frames)
    if fam.layout == dg.DXH:
        assert r.last_kernel() == capi.KERNEL_FUSED, r.last_kernel()
        bt, dt = r.process(frames, layout=dg.DXH)
    assert r.last_kernel() == want_kernel, (fam.name, r.last_kernel(), want_kernel, r.jit_note())
    if want_kernel == capi.KERNEL_WAVE_JIT:
        assert r.jit_note() == "", r.jit_note()
    if fam.setup == "staged":     # the two-kernel mode equals the fused chain bit for bit
        assert np.array_equal(_bits(b), _bits(b0)) and np.array_equal(_bits(d), _bits(d0)), "staged mode differs from the fused chain"
    if fam.layout == dg.DXH:      # the chain's own D x H store equals the transpose of its row-major result
        assert np.array_equal(_bits(bt), _bits(np.transpose(b, (0, 2, 1)))), "D x H image differs from the row-major one"
        assert np.array_equal(_bits(dt), _bits(np.transpose(d, (0, 2, 1)))), "D x H dB image differs from the row-major one"
    return b, d


def _check_case(fam, case, b, d, log, figures):
    """Every assertion of a case; the figures go to `log` and `figures` before anything is asserted."""
    what = "%s, %s" % (fam.name, case)
    tid = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    mag_o, db_o, mag_t, db_t = dg.reference(fam.name, case)
    eps = np.float32(dg.eps_of(case))
    H = fam.H
    assert b.shape == mag_o.shape and d.shape == db_o.shape
    assert np.isfinite(b).all() and np.isfinite(d).all(), what + ": non-finite output"
    empty, dc = dg.empty_rows(case, H), dg.dc_level_rows(case)
    exact = dg.exact_empty_rows(case, H)
    db_eps = np.float32((20.0 / 2.303) * np.log(np.float64(eps)))
    if exact:
        ulps = _ulps(d[0, exact], db_eps)
        log.append("%s: empty rows %s, %d bins off float32(eps), dB within %d ulp" % (what, exact, int((_bits(b[0, exact]) != _bits(eps)).sum()), ulps))
        assert np.array_equal(_bits(b[0, exact]), np.broadcast_to(_bits(eps), b[0, exact].shape)), what + ": an empty row is not float32(eps)"
        assert ulps <= 1, "%s: the dB of an empty row is %d ulp from the dB of float32(eps)" % (what, ulps)
    # (the constant rows under row-wise normalisation are among `exact`: their scale is 0)
    fb = [r for r in dc if r == dg.NO_FRINGE and dg.half_pattern(fam.name, case)]
    rows = [r for r in range(H) if r not in fb]
    g, o = helpers.truth_ratios(b[:, rows], mag_t[:, rows], mag_o[:, rows])
    helpers.TRUTH_LOG.append((tid, what, g, o))
    figures.append(g)
    log.append("%s: |gpu - truth| / tol = %.3g (f32 restatement %.3g)" % (what, g, o))
    rowmax0 = np.abs(mag_t[:, dg.ORDINARY]).max()
    if dc:
        log.append("%s: DC-level rows %s: %.3g x their own tolerance, %.3g x the tolerance at row 0's peak, max |gpu - eps| = %.3g" % (
            what, dc, helpers.truth_ratios(b[:, dc], mag_t[:, dc])[0], helpers.truth_ratios(b[:, dc], mag_t[:, dc], rowmax=rowmax0)[0],
            float(np.abs(b[0, dc].astype(np.float64) - float(dg.eps_of(case))).max())))
    helpers.check_truth(b[:, rows], mag_t[:, rows], mag_o[:, rows], what)
    helpers.check_mag(b[:, rows], mag_o[:, rows], what)
    helpers.check_db(d[:, rows], db_o[:, rows], mag_o[:, rows], what)
    if fb:
        g_fb = helpers.truth_ratios(b[:, fb], mag_t[:, fb], rowmax=rowmax0)[0]
        assert g_fb <= helpers.TRUTH_LIMIT, "%s: the no-fringe row is %.3g x the tolerance at row 0's peak from the chain in double" % (what, g_fb)
        gd = float(helpers.db_ratio(d[:, fb], db_t[:, fb], mag_t[:, fb], rowmax0).max())
        assert gd <= 1.0, "%s: the no-fringe row's dB is %.3g x the bound that tolerance implies" % (what, gd)
        # ... and what is left of the row is what the half-float pattern leaves, not more: the row that form gives in double,
        # under the rule as it stands (the row's own peak)
        model = dg.half_pattern_no_fringe_row(fam.name, case)
        g_m = helpers.truth_ratios(b[0, fb], model[None])[0]
        log.append("%s: the no-fringe row is %.3g x its own tolerance from the half-float pattern's row" % (what, g_m))
        assert g_m <= helpers.TRUTH_LIMIT, "%s: the no-fringe row is %.3g x its tolerance from what the half-float pattern leaves" % (what, g_m)
    if case.bg != "full" and case.opt in ("plain", "rowwise") and case.frames in ("one", "pair"):
        assert np.array_equal(_bits(b[0, dg.COPY]), _bits(b[0, dg.ORDINARY])), what + ": the copy of row 0 differs from row 0"
        assert np.array_equal(_bits(d[0, dg.COPY]), _bits(d[0, dg.ORDINARY])), what + ": the copy of row 0 differs from row 0 (dB)"


@pytest.mark.parametrize("name", dg.FAMILY_IDS)
def test_degenerate_frames_and_planes(name):
    fam = dg.family(name)
    handles = _Handles(fam)
    log, failures, figures = [], [], []
    try:
        for case in fam.cases:
            i = dg.inputs(name, case)
            r = handles.get(case, i)
            b, d = _run(fam, r, i.frames, dg.expected_kernel(fam, case))
            try:
                _check_case(fam, case, b, d, log, figures)
            except AssertionError as e:
                failures.append(str(e).split("\n")[0])
    finally:
        handles.close()
    print("\n".join(log))
    print("%s: worst |gpu - truth| / tol over %d cases = %.3g" % (name, len(fam.cases), max(figures, default=0.0)))
    assert not failures, "%d of %d cases:\n  " % (len(failures), len(fam.cases)) + "\n  ".join(failures)


# ---- row isolation with non-finite samples -------------------------------------------------------------------------------------------
# every family but staged mode, which refuses anything but 16-bit samples (fdoct_launch.cpp), and the D x H entries, whose
# geometries are here already: float frames reach D x H through the transpose pass, run below for every family
FLOAT_FAMILIES = [n for n in dg.FAMILY_IDS if dg.family(n).setup != "staged" and dg.family(n).layout != dg.DXH]
POISONED = dg.IMPULSE_LEFT       # row 5


@pytest.mark.parametrize("opt", ["plain", "rowwise"])
@pytest.mark.parametrize("name", FLOAT_FAMILIES)
def test_a_non_finite_row_leaves_the_other_rows_alone(name, opt):
    """The 11-row frame as floats: clean, with row 5 all NaN, and with a single +Inf in row 5.  Every other row is bit-identical to
    the clean run, linear and dB, in both layouts.  Row 5's own content is not asserted."""
    fam = dg.family(name)
    case = dg.Case(opt, "dead")
    i = dg.inputs(name, case)
    clean = i.frames.astype(np.float32)
    nan, inf = clean.copy(), clean.copy()
    nan[0, POISONED] = np.nan
    inf[0, POISONED, i.frames.shape[2] // 3] = np.inf
    others = [r for r in range(fam.H) if r != POISONED]
    r = Reconstructor(i.cfg)
    try:
        if fam.setup == "any-option":
            r.set_plan(-1, True)
        r.set_background(i.yb)
        out = {}
        for what, f in (("clean", clean), ("NaN row", nan), ("+Inf sample", inf)):
            b, d = r.process(f)
            k = r.last_kernel()
            assert k == dg.expected_kernel(fam, case), (name, k, r.jit_note())
            bt, dt = r.process(f, layout=dg.DXH)
            out[what] = (b, d, np.transpose(bt, (0, 2, 1)), np.transpose(dt, (0, 2, 1)))
        print("%s, %s: kernel %d" % (name, opt, k))
    finally:
        r.close()
    b, d, bt, dt = out["clean"]
    assert np.isfinite(b).all() and np.isfinite(d).all()
    assert np.array_equal(_bits(bt), _bits(b)) and np.array_equal(_bits(dt), _bits(d))
    mag_o, db_o, _, _ = dg.reference(name, case)
    helpers.check_mag(b, mag_o, "%s, %s, f32 frames" % (name, opt))
    for what in ("NaN row", "+Inf sample"):
        for a, c, img in zip(out[what], out["clean"], ("linear", "dB", "linear, D x H", "dB, D x H")):
            bad = np.argwhere(_bits(a[0, others]) != _bits(c[0, others]))
            assert bad.size == 0, "%s, %s, %s: %d values of the %s image outside row %d changed, first in row %d" % (
                name, opt, what, len(bad), img, POISONED, others[bad[0][0]])
