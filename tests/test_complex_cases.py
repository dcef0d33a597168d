"""CPU checks of tests/complex_cases.py, for every case tests/test_gpu_complex_options.py runs, with the reference alone
(tests/complex_model.py: the oracle's float composition and the same composition in double).

The float composition's own ratio |f32 composition - truth| / tolerance over the rows that are neither empty nor cancelled is at
most helpers.TRUTH_LIMIT on every option, phase, depth and degenerate case -- so max(TRUTH_LIMIT, the composition's own) never
widens what the GPU is allowed -- and at most resample_tables.ORACLE_LIMIT on every (family, table) pair that is run; the pairs
that are not are exactly complex_cases.DROPPED_PAIRS, one pair, and that pair is beyond the limit.  (Measured: 0.02 - 0.13 on the
cases, but 0.37 for the band-pass and 0.30 for the four-option mask on 200 x 4 -> 2560; 0.03 - 0.20 on 63 pairs, 0.364 on the
dropped one.)  The empty and the cancelled rows of every degenerate case and every table are exactly 0 in the float composition
and in double: complex_model.check_rows' two rules for them have nothing of the reference to allow for.  And the outputs are not
degenerate themselves: imaginary parts are not zero on ordinary rows, and two ordinary rows differ by more than their tolerance,
so a kernel that serves one row's result for another, or a real part alone, fails."""
import numpy as np
import pytest

import complex_cases as cc
import complex_model as cm
import degenerate_cases as dg
import helpers
import resample_tables as rt

EDGE_CASES = cc.PHASE_CASES + cc.DEPTH_CASES


def _apart(a, b):
    """max over the bins of |a - b| / (tol(a) + tol(b)) for two rows of the composition in double."""
    return float((np.abs(a - b) / (cm.tolerance(a) + cm.tolerance(b))).max())


def _own_ratio(ref, truth, rows):
    return cm.ratio(ref[:, rows], truth[:, rows]) if rows else 0.0


def test_the_case_tables_are_what_the_gpu_tests_say_they_run():
    names = [c.name for c in cc.OPTION_CASES + EDGE_CASES]
    assert len(set(names)) == len(names)
    wave = [c.kind for c in cc.OPTION_CASES if c.route == "wave"]
    generic = [c.kind for c in cc.OPTION_CASES if c.route == "generic"]
    assert wave == list(cc.KINDS) + [cc.FOUR_BITS] and generic == list(cc.KINDS) and len(cc.KINDS) == 12
    # the form a case runs is its shape's, but for the passes that hand over two float planes (doubles, tap sums of non-integer floats)
    assert all(c.family == ("generic" if c.kind in cc.LOW_WORD_KINDS else c.route) and c.name.startswith(c.family + ": ") for c in cc.OPTION_CASES)
    assert set(cc.LOW_WORD_KINDS) < set(cc.KINDS) and sum(c.family == "wave" for c in cc.OPTION_CASES) == 10
    for c in cc.OPTION_CASES:
        s = cc.option_setup(c)
        W, M, N, D = c.shape
        assert c.shape == (cc.WAVE_SHAPE if c.route == "wave" else cc.GENERIC_BANDPASS_SHAPE if c.kind == "band-pass" else cc.GENERIC_SHAPE)
        assert (s.cfg.width, s.cfg.increasefftpointsmultiplier, s.cfg.numfftpoints, s.cfg.numdisplaypoints, s.cfg.height, s.cfg.averages) == (W, M, N, D, cc.H, 1)
        assert s.model_frames.shape == (cc.NF, cc.H, W) and s.frames.shape[:3] == (cc.NF, cc.H, W)
        assert s.yb.shape == ((cc.H, W) if c.kind == "full-frame background" else (W,)) and s.yb.min() > 0
        assert bool(s.mkw.get("bandpass")) == bool(s.hkw.get("bandpass")) == (c.kind in ("band-pass", cc.FOUR_BITS)) and (not s.mkw.get("bandpass") or M > 1)
        assert s.cfg.rowwisenormalize == int(c.kind in ("rowwisenormalize", cc.FOUR_BITS))
        assert s.cfg.donotnormalize == int(c.kind != "whole-frame normalise")
        assert s.cfg.movavgn == (cc.MOVAVGN if c.kind.startswith("movavgn") else 0)
        assert ("yp" in s.mkw) == ("yd" in s.mkw) == (c.kind == cc.FOUR_BITS)
        want = {"movavgn 3, f32 non-integer frames": np.float32, "f32 frames": np.float32, "movavgn 3, f64 non-integer frames": np.float64,
                "median 3 of raw u8 frames": np.uint8, "colour handle, channel 1": np.uint8, "colour handle, channel 3": np.uint8}.get(c.kind, np.uint16)
        assert s.frames.dtype == want, c.name
        if s.frames.dtype.kind == "f":
            assert not np.any(s.frames == np.rint(s.frames)) and s.model_frames is s.frames
        if c.kind.startswith("median"):
            assert s.hkw["frontend"] == (3, 1, 1) and s.model_frames.shape == s.frames.shape and not np.array_equal(s.model_frames, s.frames)
        if c.kind.startswith("colour"):
            ch = s.hkw["colour"]
            assert s.frames.shape == (cc.NF, cc.H, W, 3) and ch in (1, 3)
            assert s.model_frames.dtype == (np.float64 if ch == 3 else np.uint8)
            if ch == 1:
                assert np.array_equal(s.model_frames, s.frames[..., 1]) and not np.array_equal(s.frames[..., 1], s.frames[..., 0])
        if c.kind == "Hamming window":
            assert abs(s.mkw["window"][0] - 0.08) < 1e-12 and s.hkw["window"] is s.mkw["window"]
    W, M, N = cc.EDGE_SHAPE
    assert cc.PHASE_DEPTHS == (N, N // 2 + 21) and all(d > N // 2 for d in cc.PHASE_DEPTHS)
    assert cc.DEPTHS == (1, 63, 64, 65, N // 2, N // 2 + 1, N)
    assert len(cc.PHASE_CASES) == 8 and len(cc.DEPTH_CASES) == 14
    for c in EDGE_CASES:
        s = cc.edge_setup(c)
        assert s.cfg.numdisplaypoints == c.D and ("phase" in s.mkw) == c.phase and (s.hkw.get("jit", True) is False) == (c.route == "generic")
    # the degenerate and the table families are entries of the modules they come from; no averaging pair among the cases
    assert set(cc.DEGENERATE_FAMILIES) <= set(dg.FAMILY_IDS) and set(cc.TABLE_FAMILIES) <= set(rt.FAMILY_IDS) and len(cc.TABLE_FAMILIES) == 8
    assert len(cc.DEGENERATE_CASES) == 10 == len(set(cc.DEGENERATE_CASES)) and all(c.frames != "pair" and c.bits == 16 for c in cc.DEGENERATE_CASES)
    for name in cc.DEGENERATE_FAMILIES:
        for case in cc.DEGENERATE_CASES + cc.ISOLATION_CASES:
            i = dg.inputs(name, case)
            assert i.cfg.averages == 1 and i.frames.shape == (1, dg.ROWS, i.cfg.width)
    assert [cc.wave_family(n) for n in cc.TABLE_FAMILIES] == [True] * 4 + [False] * 4
    assert cc.DROPPED_PAIRS == [("workgroup-per-row, full-length zero-pad, 161 x 4", "evenodd")]
    assert sum(len(cc.tables_of(n)) for n in cc.TABLE_FAMILIES) == 63 and all(tuple(rt.family(n).tables) == rt.TABLES for n in cc.TABLE_FAMILIES)


@pytest.mark.parametrize("case", cc.OPTION_CASES + EDGE_CASES, ids=[c.name for c in cc.OPTION_CASES + EDGE_CASES])
def test_the_reference_on_every_option_phase_and_depth_case(case):
    ref, truth = cc.setup_models(case)
    D = case.shape[3] if isinstance(case, cc.Option) else case.D
    assert ref.shape == truth.shape == (cc.NF, cc.H, D) and ref.dtype == np.complex64 and truth.dtype == np.complex128
    assert np.isfinite(ref.view(np.float32)).all() and np.isfinite(truth.view(np.float64)).all()
    o = cm.ratio(ref, truth)
    print("%s: |f32 composition - truth| / tol = %.4f" % (case.name, o))
    assert o <= helpers.TRUTH_LIMIT, "%s: the float composition is %.3g x the tolerance from the composition in double" % (case.name, o)
    if D > 1:     # (bin 0 of a real row is real)
        assert (np.abs(truth.imag).max(axis=-1) > cm.tolerance(truth).max(axis=-1)).all(), case.name
        assert _apart(truth[0, 0], truth[0, cc.H - 1]) > 1.0 and _apart(truth[0, 0], truth[1, 0]) > 1.0, case.name
    else:
        assert (np.abs(truth) > 0).all()


def test_the_options_change_what_the_chain_gives():
    """Every option case differs from the plain chain on its frames by more than the tolerance: an option that is not applied shows."""
    for c in cc.OPTION_CASES:
        s = cc.option_setup(c)
        plain = cc.Config(width=s.cfg.width, height=cc.H, numfftpoints=s.cfg.numfftpoints, numdisplaypoints=s.cfg.numdisplaypoints,
                          increasefftpointsmultiplier=s.cfg.increasefftpointsmultiplier)
        kind = c.kind
        if kind in ("f32 frames", "colour handle, channel 1", "colour handle, channel 3", "full-frame background"):
            continue      # (another sample type, or another background: there is no plain chain on the same inputs to differ from)
        frames = s.frames if kind.startswith("median") else s.model_frames
        base = cm.model(plain, frames, s.yb, truth=1)
        assert _apart(base[0, 0], cc.setup_models(c)[1][0, 0]) > 1.0, c.name


@pytest.mark.parametrize("name", cc.DEGENERATE_FAMILIES)
def test_the_reference_on_every_degenerate_case(name):
    for case in cc.DEGENERATE_CASES:
        what = cc.degenerate_name(name, case)
        ref, truth = cc.degenerate_models(name, case)
        i = dg.inputs(name, case)
        assert ref.shape == truth.shape == (1, dg.ROWS, i.cfg.numdisplaypoints)
        assert np.isfinite(ref.view(np.float32)).all() and np.isfinite(truth.view(np.float64)).all(), what
        empty, cancelled = cc.degenerate_rows(case)
        assert sorted(empty + cancelled) == dg.empty_rows(case) and not set(empty) & set(cancelled), what
        assert set(cancelled) <= {dg.NO_FRINGE, dg.TOP, dg.MID}
        rows = [r for r in range(dg.ROWS) if r not in empty and r not in cancelled]
        o = _own_ratio(ref, truth, rows)
        print("%s: |f32 composition - truth| / tol = %.4f; empty %s, cancelled %s" % (what, o, empty, cancelled))
        assert o <= helpers.TRUTH_LIMIT, "%s: the float composition is %.3g x the tolerance from the composition in double" % (what, o)
        # the zero rows are exactly 0, in float and in double; no other row is
        for m in (ref, truth):
            assert not np.count_nonzero(m[0, empty + cancelled]), what
            assert all(np.count_nonzero(m[0, r]) for r in rows), what
        ordinary = [r for r in (dg.ORDINARY, dg.ORDINARY_2) if r in rows]
        for r in ordinary:
            assert np.abs(truth[0, r].imag).max() > cm.tolerance(truth[0, r]).max(), what
        distinct = [r for r in dg.distinct_rows(case) if r in rows] if case.frames == "one" else rows[:2]
        for a in range(len(distinct)):
            for b in range(a + 1, len(distinct)):
                assert _apart(truth[0, distinct[a]], truth[0, distinct[b]]) > 1.0, (what, distinct[a], distinct[b])
        if cc.copy_is_exact(case):
            for m in (ref, truth):
                assert np.array_equal(m[0, dg.COPY], m[0, dg.ORDINARY]), what


@pytest.mark.parametrize("name", cc.TABLE_FAMILIES)
def test_the_reference_under_every_table(name):
    beyond = []
    for t in rt.family(name).tables:
        what = "%s, table '%s'" % (name, t)
        ref, truth = cc.table_models(name, t)
        assert np.isfinite(ref.view(np.float32)).all() and np.isfinite(truth.view(np.float64)).all(), what
        rows = [r for r in range(dg.ROWS) if r not in cc.TABLE_EMPTY + cc.TABLE_CANCELLED]
        o = _own_ratio(ref, truth, rows)
        print("%s: |f32 composition - truth| / tol = %.4f" % (what, o))
        if o > rt.ORACLE_LIMIT:
            beyond.append((name, t))
        for m in (ref, truth):
            assert not np.count_nonzero(m[0, cc.TABLE_EMPTY + cc.TABLE_CANCELLED]), what
            assert all(np.count_nonzero(m[0, r]) for r in rows), what
            assert np.array_equal(m[0, dg.COPY], m[0, dg.ORDINARY]), what
        for r in (dg.ORDINARY, dg.ORDINARY_2):
            assert np.abs(truth[0, r].imag).max() > cm.tolerance(truth[0, r]).max(), what
        assert _apart(truth[0, dg.ORDINARY], truth[0, dg.ORDINARY_2]) > 1.0, what
    # the pairs beyond the limit are the dropped ones of this family, no more and no fewer
    assert beyond == [p for p in cc.DROPPED_PAIRS if p[0] == name], beyond
    assert cc.tables_of(name) == [t for t in rt.family(name).tables if (name, t) not in beyond]
    assert dg.exact_empty_rows(rt.CASE) == cc.TABLE_EMPTY and dg.dc_level_rows(rt.CASE) == cc.TABLE_CANCELLED
