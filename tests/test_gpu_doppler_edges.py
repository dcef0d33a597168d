"""GPU tests of the Doppler stage alone (fdoct_doppler: doppler_kernel, doppler_bulk_kernel) where tests/test_gpu_doppler.py does
not go, on the cases of tests/doppler_edge_cases.py (held to their conditions on the CPU by tests/test_doppler_edge_cases.py):

  a. tile seams: pair rows 15 .. 33 x depths 63 .. 129 around the 16 x 64 tile, where the last tile's halo is cut at the image and
     not at the tile; 4 x 8 on the A-scans axis, 3 x 5 with the bulk correction on the frames axis;
  b. every window size 1 .. 32 each way, the anti-diagonal, 2 x 2 and 31 x 31, and the two sizes either side of 64 KiB of LDS;
  c. reach: one sample made NaN changes exactly the outputs whose window holds a pair formed from it -- the halo, the "pairs
     outside the image are not loaded" rule and the lag partner, seen directly and bit for bit;
  d. a batch beyond one pass of the capped grid whose pair images have two tiles each way;
  e. the mask's strict comparison on a field whose every product and sum is exact in float;
  f. three device calls back to back with one synchronise, the middle one growing the handle's phasor buffer, and input pairs
     that are only 8-byte aligned.

Comparisons with a tolerance go through doppler_model.check (the derived bound, adjudicated against the composition in double,
the ratios appended to helpers.TRUTH_LOG); every other comparison is bit for bit or an exact known value.  When
FDOCT_DOPPLER_EDGES_TABLE names a file the ratios go into it (profiles/doppler_edges_truth_table.txt is such a run)."""
import os

import numpy as np
import pytest

import doppler_cases as dc
import doppler_edge_cases as de
import doppler_model as dm
from fdoct_amd import Config, Reconstructor
from test_gpu_doppler import NAMES, _bits, _device, _raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    r = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=32))   # the stage reads nothing of the geometry
    yield r
    r.close()


@pytest.fixture(scope="module", autouse=True)
def _table():
    first = len(dm.RATIOS)
    yield
    path = os.environ.get("FDOCT_DOPPLER_EDGES_TABLE")
    if path and len(dm.RATIOS) > first:
        with open(path, "w") as f:
            f.write("# case | corr |gpu - truth| / tol_R | corr |f32 model - truth| / tol_R | power |gpu - truth| / tol_P | power |f32 model - truth| / tol_P |\n")
            f.write("# worst phase error / PHASE_TOL   (tests/doppler_model.py: check)\n")
            for what, gR, oR, gP, oP, ph in dm.RATIOS[first:]:
                f.write("%-72s %.4f  %.4f  %.4f  %.4f  %.4f\n" % (what, gR, oR, gP, oP, ph))


def _run(rec, X, kw):
    """The stage on host memory into NaN-poisoned outputs."""
    rc, out = _raw(rec, X, **kw)
    assert rc == 0, rec.lib.fdoct_last_error(rec.h)
    return out


def _check(rec, X, kw, what):
    out = _run(rec, X, kw)
    dm.check(out, X, kw["axis"], kw["lag"], what, kw["win"], kw["bulk"], kw["scale"], kw["min_power"])   # (finite everywhere: no poison left)
    return out


# ---- a. seams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", de.SEAM_CASES + de.SEAM_BULK_CASES, ids=[c["what"] for c in de.SEAM_CASES + de.SEAM_BULK_CASES])
def test_tile_seams(rec, case):
    _check(rec, dc.case_field(case), dc.case_args(case), case["what"])


# ---- b. every window size ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(de.WINDOW_GROUPS))
def test_every_window_size(rec, group):
    X = de.sweep_field()
    name = "%d x %d x %d" % de.SWEEP_SHAPE
    failures = []
    for win in de.WINDOW_GROUPS[group]:
        try:
            _check(rec, X, de.sweep_args(win), "%d x %d, %s" % (win[0], win[1], name))
        except AssertionError as e:
            failures.append("%d x %d: %s" % (win[0], win[1], str(e).split("\n")[0]))
    if tuple(de.WINDOW_GROUPS[group]) == de.LDS_STRADDLE:   # 65 520 B, then 65 940 B (the raised limit), then the smallest tile again
        try:
            _check(rec, X, de.sweep_args((1, 1)), "1 x 1 after 20 x 30, " + name)
        except AssertionError as e:
            failures.append("1 x 1 after 20 x 30: " + str(e).split("\n")[0])
    assert not failures, "%d of %d windows:\n  " % (len(failures), len(de.WINDOW_GROUPS[group])) + "\n  ".join(failures)


# ---- c. reach ------------------------------------------------------------------------------------------------------------------------
def _nan(a):
    return np.isnan(a.real) | np.isnan(a.imag) if np.iscomplexobj(a) else np.isnan(a)


@pytest.mark.parametrize("cfg", de.reach_configs(), ids=lambda c: "axis %d, lag %d, %d x %d" % (c[0], c[1], c[2][0], c[2][1]))
def test_a_sample_reaches_exactly_the_windows_that_hold_its_pairs(rec, cfg):
    """One sample of a clean 34 x 130 field is made NaN: at the four corners of the interior tile seam and at the image's first
    and last sample.  Outside the sample's reach (doppler_edge_cases.reach) all three images keep the clean run's bits; inside
    it correlation and power are NaN.

    With the bulk correction only the rows out of reach of the sample's pair rows are asserted to keep their bits.  Observed on
    the MI355X: the poisoned pair row's sum B is NaN, `m > 0` is false and its phasor is the documented fallback (1, 0), so that
    row's terms go unturned and the correlation changes at every depth of the rows whose window holds it -- finite outside the
    sample's own depth span, NaN inside it -- while the power, which the phasor does not enter, keeps its bits outside the
    plain reach."""
    axis, lag, win = cfg
    X = de.reach_field(axis, lag)
    kw = dict(axis=axis, lag=lag, win=win, bulk=None, scale=1.0, min_power=0.0)
    clean = _check(rec, X, kw, "reach's clean field, axis %d, lag %d, %d x %d" % (axis, lag, win[0], win[1]))
    clean_bulk = _run(rec, X, dict(kw, bulk=True))
    for pos in de.reach_positions(axis, lag):
        Y = de.poisoned(X, pos)
        got = _run(rec, Y, kw)
        hit = de.reach(axis, lag, win, pos, X.shape)
        assert hit.any() and not hit.all()
        for w in NAMES:
            changed = (_bits(got[w]) != _bits(clean[w])).reshape(hit.shape + (-1,)).any(-1)
            assert not (changed & ~hit).any(), "%s: %d bins outside the reach of sample %s changed, first at %s" % (
                w, (changed & ~hit).sum(), pos, tuple(np.argwhere(changed & ~hit)[0]))
        for w in ("corr", "power"):
            assert np.array_equal(_nan(got[w]), hit), "%s: NaN in %d bins, the reach of sample %s has %d" % (w, _nan(got[w]).sum(), pos, hit.sum())
        got = _run(rec, Y, dict(kw, bulk=True))
        rows = de.reach(axis, lag, win, pos, X.shape, all_depths=True)
        for w in NAMES:
            changed = (_bits(got[w]) != _bits(clean_bulk[w])).reshape(rows.shape + (-1,)).any(-1)
            assert not (changed & ~rows).any(), "bulk, %s: %d bins in rows out of reach of sample %s changed" % (w, (changed & ~rows).sum(), pos)
        print("bulk, sample %s: corr changed in %d bins of the %d in reach of its rows, %d of them NaN; power in %d, the plain reach has %d" % (
            pos, (_bits(got["corr"]) != _bits(clean_bulk["corr"])).reshape(rows.shape + (-1,)).any(-1).sum(), rows.sum(), _nan(got["corr"]).sum(),
            (_bits(got["power"]) != _bits(clean_bulk["power"])).sum(), hit.sum()))


# ---- d. a tall batch with tiles both ways --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [dm.ASCANS, dm.FRAMES], ids=["A-scans, bulk", "frames"])
def test_a_tall_batch_of_two_by_two_tiles_repeats_its_base_bit_for_bit(rec, axis):
    """Frames of 18 x 65, two row tiles x two depth tiles a pair image, so that the grid's second pass decodes tiles with
    tiles_r = tiles_d = 2: pair image p of the tall result equals pair image p mod 3 of the base's, bit for bit."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    base_n, lag = de.TALL2_BASE[axis]
    n = de.tall2_frames(axis, cus)
    assert de.tall2_ok(axis, n, cus) and de.tall2_base_ok(axis, cus)
    three = dc.field(3, de.TALL2_H, de.TALL2_D, 500, speckle=True)
    kw = dict(axis=axis, lag=lag, win=de.TALL2_WIN, bulk=de.TALL2_BULK[axis], scale=1.0, min_power=0.0)
    base = np.ascontiguousarray(three[np.arange(base_n) % 3])
    want = _check(rec, base, kw, "2 x 2-tile tall batch's base, axis %d" % axis)
    tall = np.ascontiguousarray(three[np.arange(n) % 3])
    got = _device(rec, tall, kw)
    pi = dm.pair_shape(axis, lag, n, de.TALL2_H)[0]
    for w in NAMES:
        np.testing.assert_array_equal(_bits(got[w]), _bits(want[w][np.arange(pi) % 3]), err_msg="%s, %d frames on %d CUs" % (w, n, cus))


# ---- e. the mask is strict -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", de.EXACT_WINDOWS, ids=lambda w: "%d x %d" % w)
def test_the_mask_is_strict_on_an_exact_field(rec, win):
    """X = (3 + 4j) i^r: power is exactly 25 in every bin and corr exactly (0, 25 cnt).  min_power = 25 masks nothing (the header:
    0 where P / cnt < min_power); one ulp above it masks every bin and moves no other bit."""
    X = de.exact_field()
    cnt = dm.count(X.shape[1] - 1, X.shape[2], *win)
    kw = dict(axis=dm.ASCANS, lag=1, win=win, bulk=None, scale=1.0)
    at = _run(rec, X, dict(kw, min_power=de.EXACT_POWER))
    assert np.all(at["power"] == np.float32(de.EXACT_POWER)), "%d x %d: power is not 25 everywhere" % win
    assert np.all(at["corr"].real == 0) and np.all(at["corr"].imag == (de.EXACT_POWER * cnt).astype(np.float32)[None]), "%d x %d: corr is not (0, 25 cnt)" % win
    off = np.abs(at["phase"].astype(np.float64) - np.pi / 2)
    print("%d x %d: phase - pi / 2 within %.3g rad; %d bins are float32(pi / 2) exactly" % (win + (off.max(), (at["phase"] == np.float32(np.pi / 2)).sum())))
    assert np.all(off <= dm.PHASE_TOL), "%d x %d: %d bins at min_power are masked or off pi / 2 by up to %.3g rad" % (win + ((off > dm.PHASE_TOL).sum(), off.max()))
    free = _run(rec, X, dict(kw, min_power=0.0))
    for w in NAMES:
        np.testing.assert_array_equal(_bits(at[w]), _bits(free[w]), err_msg="%s with min_power = 25 against no mask" % w)
    above = _run(rec, X, dict(kw, min_power=float(np.nextafter(np.float32(de.EXACT_POWER), np.float32(np.inf)))))
    assert np.all(_bits(above["phase"]) == 0), "%d x %d: %d bins one ulp below min_power are not +0" % (win + (np.count_nonzero(_bits(above["phase"])),))
    for w in ("corr", "power"):
        np.testing.assert_array_equal(_bits(above[w]), _bits(at[w]), err_msg=w)


# ---- f. back to back on the device ---------------------------------------------------------------------------------------------------
def _enqueue(rec, X, kw, in_off=0):
    """doppler_device without a synchronise: the input `in_off` bytes past a 16-byte boundary, NaN-filled outputs.  Returns what
    keeps the buffers alive and reads them back."""
    import torch
    n, H, D = X.shape
    pi, pr = dm.pair_shape(kw["axis"], kw["lag"], n, H)
    bins = pi * pr * D
    flat = np.ascontiguousarray(X).view(np.float32).reshape(-1)
    d_in = torch.zeros(flat.size + 4, dtype=torch.float32, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and in_off % 8 == 0
    d_in[in_off // 4:in_off // 4 + flat.size] = torch.from_numpy(flat).cuda()
    bufs = {w: torch.full(((2 if w == "corr" else 1) * bins,), float("nan"), dtype=torch.float32, device="cuda") for w in NAMES}
    torch.cuda.synchronize()

    def launch():
        rec.doppler_device(d_in.data_ptr() + in_off, n, H, D, kw["axis"], kw["lag"], bufs["phase"].data_ptr(), bufs["corr"].data_ptr(),
                           bufs["power"].data_ptr(), win=kw["win"], bulk=kw["bulk"], scale=kw["scale"], min_power=kw["min_power"])

    def read():
        out = {w: bufs[w].cpu().numpy() for w in NAMES}
        out["corr"] = out["corr"].view(np.complex64)
        return {w: a.reshape(pi, pr, D) for w, a in out.items()}

    return launch, read, d_in


def test_three_device_calls_back_to_back_with_one_synchronise(rec):
    """A small batch with the bulk correction, one with more pair rows (the handle's phasor buffer grows while the first call
    may still be running), the first again into fresh buffers; one synchronise after the third.  Each equals the same call made
    alone from host memory, bit for bit; so does the first with its input 8 bytes past a 16-byte boundary."""
    fresh = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=32))    # its phasor buffer starts empty
    try:
        small, large = dc.field(2, 18, 65, 600, speckle=True), dc.field(3, 40, 130, 601, speckle=True)
        kw = dict(axis=dm.ASCANS, lag=1, win=(4, 8), bulk=True, scale=1.0, min_power=0.0)
        calls = [_enqueue(fresh, X, kw) for X in (small, large, small)]
        for launch, _, _ in calls:
            launch()
        fresh.synchronize()
        got = [read() for _, read, _ in calls]
        launch, read, _ = _enqueue(fresh, small, kw, in_off=8)
        launch()
        fresh.synchronize()
        got.append(read())
    finally:
        fresh.close()
    alone = {id(X): _check(rec, X, kw, "back to back, %d x %d x %d alone" % X.shape) for X in (small, large)}
    for what, X, g in zip(("first", "second, more pair rows", "third, the first again", "input 8 bytes past a 16-byte boundary"), (small, large, small, small), got):
        for w in NAMES:
            np.testing.assert_array_equal(_bits(g[w]), _bits(alone[id(X)][w]), err_msg="%s: %s" % (what, w))
