"""Every kernel family of the reconstruction chain on the caller-supplied lambda -> k resample tables of tests/resample_tables.py
(fdoct_set_resample_table, fdoct_set_lambda_range): tables that gather sample 0 and the last sample of the row, run up the row,
jump across it, wrap four times, repeat sources and extrapolate -- none of which a table the library builds itself ever does --
and the first of them again under a Hamming window, whose non-zero ends let sample 0 weigh 10 - 200 x the tolerance.
What they reach is written out separately in every family: the slopes[0] = slopes[1] rule (main:1161) as the fused kernels' planes
and first-lane feed, the wave-per-row kernel's lane-0 slope, the workgroup-per-row and long-row kernels' i == 0 branch; the column
M W - 1 that an odd width under an even multiplier does not have; the packed 16-bit gather sources, the split staging layout and
the padded and ragged rows; fractionalk indexed by sample, 0 past its end, outside [0, 1].  tests/test_resample_tables.py holds
the tables and the oracle to their conditions on the same pairs.

Per family and table: the expected kernel family (a custom table moves no configuration to another route), every output finite,
helpers.check_truth against the chain in double, helpers.check_mag / check_db against the f32 restatement, the all-zero row equal
to float32(eps) bit for bit, the copy of row 0 equal to row 0 bit for bit, and fdoct_get_resample_table returning what was set.
One handle takes a family's tables one after the other.  The no-fringe row (row 4: empty only because a DC level cancels) of the
kernels that take the second word of 1/background as a half-float pattern is held, as in tests/test_gpu_degenerate_inputs.py, to
the tolerance at the peak of row 0.

The setters' own contract: a table set after the first call gives what a fresh handle given it before its first call gives, bit
for bit, and fdoct_set_lambda_range goes back to the built table; the table travels through fdoct_export_state /
fdoct_import_state / fdoct_clone_to_device; refused tables and ranges leave outputs and table as they were; and in staged mode
fdoct_get_ylin shows the resample stage's own output, data_ylin[1] read from sample 0 among it."""
import dataclasses

import numpy as np
import pytest

import degenerate_cases as dg
import helpers
import oracle_lib as orc
import resample_tables as rt
from fdoct_amd import FdoctError, Reconstructor, build_resample_table, capi

pytestmark = pytest.mark.gpu

# the fused complex path runs the fast-path kernel of its plan with the half-float pattern as the real 1024-point plan does
HALF_PATTERN_TOO = ("fused, complex rows, 2048 -> 2048, D 700",)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _handle(fam, i, cfg=None, background=True):
    r = Reconstructor(cfg or i.cfg)
    if fam.setup == "any-option":
        r.set_plan(-1, True)
    if fam.setup == "rows-in-hbm":
        r.set_plan(-3)
    if background:
        r.set_background(i.yb)
        if i.phase is not None:
            r.set_dispersion_phase(i.phase)
    return r


def _give(r, fam_name, t):
    r.set_window(rt.window(t, rt.shape(rt.family(fam_name))[0]))      # (None: the built window again)
    if t == "wide":
        r.set_lambda_range(*rt.WIDE_RANGE)
    else:
        r.set_resample_table(*rt.family_table(fam_name, t))


def _run(fam, r, frames):
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
    assert r.last_kernel() == fam.kernel, (fam.name, r.last_kernel(), fam.kernel, r.jit_note())
    if fam.kernel == capi.KERNEL_WAVE_JIT:
        assert r.jit_note() == "", r.jit_note()
    if fam.setup == "staged":     # the two-kernel mode equals the fused chain bit for bit
        assert _same(b, b0) and _same(d, d0), "staged mode differs from the fused chain"
    if fam.layout == dg.DXH:      # the chain's own D x H store equals the transpose of its row-major result
        assert _same(bt, np.transpose(b, (0, 2, 1))), "D x H image differs from the row-major one"
        assert _same(dt, np.transpose(d, (0, 2, 1))), "D x H dB image differs from the row-major one"
    return b, d


def _check(fam, t, b, d, log):
    """Every assertion of a (family, table) pair; the figure goes to `log` before anything is asserted.  Returns it."""
    what = "%s, table '%s'" % (fam.name, t)
    mag_o, db_o, mag_t, db_t = rt.reference(fam.name, t)
    assert b.shape == mag_o.shape and d.shape == db_o.shape
    half = (fam.name in dg.FAMILY_IDS and dg.half_pattern(fam.name, rt.CASE)) or fam.name in HALF_PATTERN_TOO
    rows = [r for r in range(fam.H) if not (half and r == dg.NO_FRINGE)]
    g, o = helpers.truth_ratios(b[:, rows], mag_t[:, rows], mag_o[:, rows])
    helpers.TRUTH_LOG.append(("test_gpu_resample_tables", what, g, o))
    log.append("%s: |gpu - truth| / tol = %.3g (f32 restatement %.3g)" % (what, g, o))
    assert np.isfinite(b).all() and np.isfinite(d).all(), what + ": non-finite output"
    helpers.check_truth(b[:, rows], mag_t[:, rows], mag_o[:, rows], what)
    helpers.check_mag(b[:, rows], mag_o[:, rows], what)
    helpers.check_db(d[:, rows], db_o[:, rows], mag_o[:, rows], what)
    if half:
        rowmax0 = np.abs(mag_t[:, dg.ORDINARY]).max()
        fb = [dg.NO_FRINGE]
        g_fb = helpers.truth_ratios(b[:, fb], mag_t[:, fb], rowmax=rowmax0)[0]
        assert g_fb <= helpers.TRUTH_LIMIT, "%s: the no-fringe row is %.3g x the tolerance at row 0's peak from the chain in double" % (what, g_fb)
    eps = np.float32(dg.eps_of(rt.CASE))
    assert np.array_equal(_bits(b[0, dg.ZEROS]), np.broadcast_to(_bits(eps), b[0, dg.ZEROS].shape)), what + ": the all-zero row is not float32(eps)"
    assert _same(b[0, dg.COPY], b[0, dg.ORDINARY]) and _same(d[0, dg.COPY], d[0, dg.ORDINARY]), what + ": the copy of row 0 differs from row 0"
    return g


# ---- a. parity, per family and table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rt.FAMILY_IDS)
def test_every_family_on_custom_tables(name):
    fam = rt.family(name)
    W, M, N, _ = rt.shape(fam)
    i = rt.inputs(name)
    log, failures, figures = [], [], {}
    r = _handle(fam, i)
    try:
        for t in fam.tables:
            _give(r, name, t)
            b, d = _run(fam, r, i.frames)
            try:
                got = r.get_resample_table()
                want = build_resample_table(W, M, N, *rt.WIDE_RANGE) if t == "wide" else rt.family_table(name, t)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), \
                    "%s, table '%s': fdoct_get_resample_table does not return it" % (name, t)
                figures[t] = _check(fam, t, b, d, log)
            except AssertionError as e:
                failures.append(str(e).split("\n")[0])
    finally:
        r.close()
    print("\n".join(log))
    print("%s: worst |gpu - truth| / tol over %d tables = %.3g" % (name, len(fam.tables), max(figures.values(), default=0.0)))
    assert not failures, "%d of %d tables:\n  " % (len(failures), len(fam.tables)) + "\n  ".join(failures)


# ---- b. the setter invalidates every table set ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rt.SETTER_FAMILIES)
def test_a_table_set_after_the_first_call_equals_one_set_before_it(name):
    fam = rt.family(name)
    W, M, N, _ = rt.shape(fam)
    i = rt.inputs(name)
    ends = rt.family_table(name, "ends")
    r, fresh = _handle(fam, i), _handle(fam, i)
    try:
        b_def, d_def = _run(fam, r, i.frames)
        r.set_resample_table(*ends)
        b_ends, d_ends = _run(fam, r, i.frames)
        fresh.set_resample_table(*ends)
        b_fresh, d_fresh = _run(fam, fresh, i.frames)
        assert not _same(b_ends[0, dg.ORDINARY], b_def[0, dg.ORDINARY]), name + ": the table changed nothing"
        assert _same(b_ends, b_fresh) and _same(d_ends, d_fresh), name + ": a table set after the first call differs from one set before it"
        r.set_lambda_range(i.cfg.lambdamin, i.cfg.lambdamax)
        b_back, d_back = _run(fam, r, i.frames)
        assert _same(b_back, b_def) and _same(d_back, d_def), name + ": fdoct_set_lambda_range did not bring the built table back"
        got, want = r.get_resample_table(), build_resample_table(W, M, N, i.cfg.lambdamin, i.cfg.lambdamax)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    finally:
        r.close()
        fresh.close()


# ---- c. read-back and state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused fast path, 1024-point plan", "wave-per-row, 160 x 4"])
def test_a_custom_table_travels_with_the_state(name):
    fam = rt.family(name)
    i = rt.inputs(name)
    saw = rt.family_table(name, "sawtooth")
    src = _handle(fam, i)
    twin = clone = None
    try:
        src.set_resample_table(*saw)
        got = src.get_resample_table()
        assert np.array_equal(got[0], saw[0]) and np.array_equal(got[1].view(np.uint64), saw[1].view(np.uint64))
        b, d = _run(fam, src, i.frames)
        twin = _handle(fam, i, background=False)
        twin.import_state(src.export_state())
        clone = src.clone_to_device(0)
        for other, how in ((twin, "fdoct_import_state"), (clone, "fdoct_clone_to_device")):
            got = other.get_resample_table()
            assert np.array_equal(got[0], saw[0]) and np.array_equal(got[1].view(np.uint64), saw[1].view(np.uint64)), (name, how)
            bo, do = _run(fam, other, i.frames)
            assert _same(bo, b) and _same(do, d), "%s: the output after %s differs from the source handle's" % (name, how)
        # ... and so does the built table's return: the flag travels, not only the arrays
        src.set_lambda_range(i.cfg.lambdamin, i.cfg.lambdamax)
        b_def, _ = _run(fam, src, i.frames)
        twin.import_state(src.export_state())
        assert _same(_run(fam, twin, i.frames)[0], b_def) and not _same(b_def, b)
    finally:
        for h in (src, twin, clone):
            if h is not None:
                h.close()


# ---- d. fdoct_set_lambda_range ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused fast path, 1024-point plan", "wave-per-row, 160 x 4"])
def test_set_lambda_range_equals_a_handle_created_with_the_range(name):
    fam = rt.family(name)
    i = rt.inputs(name)
    assert (i.cfg.lambdamin, i.cfg.lambdamax) == (816e-9, 884e-9)
    r = _handle(fam, i)
    born = _handle(fam, i, cfg=dataclasses.replace(i.cfg, lambdamin=rt.WIDE_RANGE[0], lambdamax=rt.WIDE_RANGE[1]))
    try:
        b_def, _ = _run(fam, r, i.frames)
        r.set_lambda_range(*rt.WIDE_RANGE)
        b, d = _run(fam, r, i.frames)
        bb, db = _run(fam, born, i.frames)
        assert _same(b, bb) and _same(d, db), name + ": set to 400-1000 nm differs from created with 400-1000 nm"
        assert not _same(b, b_def)
        t0, t1 = r.get_resample_table(), born.get_resample_table()
        assert np.array_equal(t0[0], t1[0]) and np.array_equal(t0[1].view(np.uint64), t1[1].view(np.uint64))
        for lo, hi in ((884e-9, 816e-9), (850e-9, 850e-9), (0.0, 884e-9), (-816e-9, 884e-9)):
            with pytest.raises(FdoctError):
                r.set_lambda_range(lo, hi)
            t2 = r.get_resample_table()
            assert np.array_equal(t2[0], t0[0]) and np.array_equal(t2[1].view(np.uint64), t0[1].view(np.uint64)), (lo, hi)
            b2, d2 = _run(fam, r, i.frames)
            assert _same(b2, b) and _same(d2, d), "%s: a refused range (%g, %g) changed the output" % (name, lo, hi)
    finally:
        r.close()
        born.close()


# ---- e. refusals of the table setter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rt.SETTER_FAMILIES)
def test_refused_tables_leave_the_handle_alone(name):
    fam = rt.family(name)
    W, M, N, _ = rt.shape(fam)
    i = rt.inputs(name)
    ends = rt.family_table(name, "ends")
    r = _handle(fam, i)
    try:
        r.set_resample_table(*ends)
        b, d = _run(fam, r, i.frames)
        low, high = ends[0].copy(), ends[0].copy()
        low[N // 2] = -1
        high[N // 2] = M * W
        for what, idx, frac in (("length N - 1", ends[0][:N - 1], ends[1][:N - 1]), ("an index of -1", low, ends[1]), ("an index of M W", high, ends[1])):
            with pytest.raises(FdoctError):
                r.set_resample_table(idx, frac)
            got = r.get_resample_table()
            assert np.array_equal(got[0], ends[0]) and np.array_equal(got[1].view(np.uint64), ends[1].view(np.uint64)), (name, what)
            b2, d2 = _run(fam, r, i.frames)
            assert _same(b2, b) and _same(d2, d), "%s: a refused table (%s) changed the output" % (name, what)
    finally:
        r.close()


# ---- f. the resample stage seen directly -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ["ends", "sawtooth", "ends+hamming"])
def test_get_ylin_under_a_custom_table(t):
    """Staged mode, 2048 -> 2048: fdoct_get_ylin against the oracle's data_ylin under test_get_ylin_matches_the_oracles_data_ylin's
    rule, 4e-6 x the row's largest |data_ylin|; data_ylin[1] -- under `ends` the output that reads sample 0 -- is not zero wherever
    the oracle's is not.  Every row but the no-fringe one, whose data_ylin is zero only because a DC level cancels (the half-float
    pattern of this kernel leaves 2^-35 of it; tests/test_gpu_degenerate_inputs.py)."""
    name = "fused, staged"
    fam = rt.family(name)
    W, M, N, D = rt.shape(fam)
    i = rt.inputs(name)
    idx, frac = rt.family_table(name, t)
    p = orc.make_params(W, fam.H, N, D)
    win = rt.window(t, W)
    want = orc.frame_to_mag(p, i.frames[0].astype(np.float64), i.yb, None, orc.barthann(W) if win is None else win, idx, frac, want_ylin=True)[1]
    r = _handle(fam, i)
    try:
        r.set_staged(True)
        _give(r, name, t)
        r.process(i.frames)
        assert r.last_kernel() == capi.KERNEL_FUSED_STAGED
        got = r.get_ylin(0, fam.H)
    finally:
        r.close()
    rows = [x for x in range(fam.H) if x != dg.NO_FRINGE]
    got, want = got[rows], want[rows]
    scale = np.abs(want).max(axis=-1, keepdims=True)
    print("get_ylin, table '%s': worst |gpu - oracle| / (4e-6 rowmax) = %.3g; data_ylin[1] of rows 0 and 9: %r against %r" % (
        t, float((np.abs(got - want) / np.maximum(4e-6 * scale, 1e-300)).max()), got[[0, rows.index(dg.ORDINARY_2)], 1], want[[0, rows.index(dg.ORDINARY_2)], 1]))
    assert (np.abs(got - want) <= 4e-6 * scale).all(), (np.abs(got - want) / np.maximum(scale, 1e-300)).max()
    assert (got[..., 0] == 0).all() and (got[..., N - 1] == 0).all()
    live = np.abs(want[:, 1]) > 4e-6 * scale[:, 0]
    assert live[0] and live[rows.index(dg.ORDINARY_2)] and (got[live, 1] != 0).all()
