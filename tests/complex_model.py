"""The specification of the complex A-scan (include/fdoct_complex.h) from the oracle's own pieces, and the rule the library is held
to.  Nothing under oracle/ changes for it.

The value is the content of `complexI` after cv::dft(..., DFT_ROWS | DFT_INVERSE) (BscanFFT.cpp:1185) and before split /
magnitude (1189-1190).  The oracle states it as a composition:

    data_ylin   orc_frame_to_mag(..., ylin_dbg): the chain up to the k-linear row, in double (every option in front of the
                transform is the oracle's own: smoothmovavg, dark and pi frame, both normalisations, zero-pad, band-pass,
                window, tables);
    z           (float)data_ylin (main:1181), times the float phasor where a dispersion phase is set, component by component
                (fdoct_oracle.c:608-614);
    X           orc_dft_rows_f32(z), inverse, unscaled; the first numdisplaypoints bins.

Its modulus is the oracle's magI bit for bit (tests/test_complex_model.py).  The truth form is the same composition with every
float step in double: orc_frame_to_mag_f64's data_ylin, the phasors promoted, orc_dft_rows_f64.

The tolerance is the project's (helpers.RTOL, helpers.ATOL_ROWMAX), applied to complex moduli:

    |gpu - ref| <= RTOL |ref| + ATOL_ROWMAX rowmax|ref|          rowmax over the A-scan's displayed bins,

and the adjudication is helpers.check_truth's: |gpu - truth| / tol <= max(helpers.TRUTH_LIMIT, the f32 composition's own
ratio).  TRUTH_LIMIT's triangle-inequality argument holds for moduli of complex differences unchanged -- two values each within
half the tolerance of the truth lie within the tolerance of each other -- and a magnitude's error is the radial part of this
one, so a result that passes here passes the magnitude rule.  Every comparison appends to helpers.TRUTH_LOG, so the suite's
truth table lists it; the worst ratios of a case are also kept in RATIOS for profiles/complex_truth_table.txt.

check_rows() is the same rule for frames that hold rows whose composition is exactly 0 (tests/degenerate_cases.py): there the
tolerance above is 0, and the rows are held to 0 or to the chain's epsilon instead -- see its docstring."""
import os

import numpy as np

import helpers
import oracle_lib as orc
from fdoct_amd import VARIANT_SIM

RATIOS = []   # (what, |gpu - f32 model| / tol, |gpu - truth| / tol, |f32 model - truth| / tol), one per check()


def _params(cfg, bandpass, truth):
    sim = cfg.variant == VARIANT_SIM
    return orc.make_params(cfg.width, cfg.height, cfg.numfftpoints, cfg.numdisplaypoints, cfg.increasefftpointsmultiplier,
                           rowwisenormalize=cfg.rowwisenormalize, donotnormalize=0 if sim else cfg.donotnormalize, movavgn=cfg.movavgn,
                           bandpass=bandpass, truth=truth)


def model(cfg, frames, yb, yp=None, yd=None, window=None, table=None, phase=None, bandpass=0, truth=0, want_mag=False):
    """X[frame][row][b], b < numdisplaypoints: complex64 (the oracle's float composition) or, truth=1, complex128.  frames:
    (n, H, W) of any real type -- data_y as main:987 holds it, after the front end.  want_mag: also the oracle's own magI
    (n, H, N) of the same frames (float32, or float64 in truth mode)."""
    W, N, D, M = cfg.width, cfg.numfftpoints, cfg.numdisplaypoints, cfg.increasefftpointsmultiplier
    p = _params(cfg, bandpass, truth)
    win = orc.barthann(W) if window is None else np.asarray(window, np.float64)
    idx, frac = orc.tables(W, M, N, cfg.lambdamin, cfg.lambdamax) if table is None else table
    ph = None if phase is None else np.ascontiguousarray(phase, np.float32).reshape(N, 2)
    out, mags = [], []
    for f in np.asarray(frames):
        mag, ylin = orc.frame_to_mag(p, np.asarray(f, np.float64), yb, yp, win, idx, frac, yd=yd, phase=ph, want_ylin=True)
        if truth:
            z = ylin.astype(np.complex128) if ph is None else ylin * ph[:, 0].astype(np.float64) + 1j * (ylin * ph[:, 1].astype(np.float64))
            X = orc.dft_rows_f64(z, inverse=True, scale=False)
        else:
            v = ylin.astype(np.float32)                                       # main:1181
            z = np.zeros(v.shape, np.complex64)
            z.real = v if ph is None else v * ph[:, 0]                        # float products, one per component
            if ph is not None:
                z.imag = v * ph[:, 1]
            X = orc.dft_rows_f32(z, inverse=True, scale=False)                # main:1185
        out.append(X[:, :D])
        mags.append(mag)
    X = np.stack(out)
    return (X, np.stack(mags)) if want_mag else X


def tolerance(ref):
    """RTOL |ref| + ATOL_ROWMAX rowmax|ref| per bin, of complex moduli; rowmax over the last axis (one A-scan's displayed bins)."""
    a = np.abs(np.asarray(ref, np.complex128))
    return helpers.RTOL * a + helpers.ATOL_ROWMAX * a.max(axis=-1, keepdims=True)


def ratio(got, ref):
    """Worst |got - ref| / tolerance(ref)."""
    got, ref = np.asarray(got, np.complex128), np.asarray(ref, np.complex128)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / np.maximum(tolerance(ref), 1e-300)).max())


def check(gpu, cfg, frames, yb, what, **kw):
    """gpu: (n, H, D) complex64 in the row-major layout.  Parity with the float composition within the tolerance, and the
    adjudication against the truth composition; every figure is printed before anything is asserted.  Returns the three ratios."""
    gpu = np.asarray(gpu)
    assert gpu.dtype == np.complex64 and np.isfinite(gpu.view(np.float32)).all(), what + ": not finite complex64"
    ref = model(cfg, frames, yb, **kw)
    truth = model(cfg, frames, yb, truth=1, **kw)
    par, g, o = ratio(gpu, ref), ratio(gpu, truth), ratio(ref, truth)
    print("%s: |gpu - f32 model| / tol = %.4f, |gpu - truth| / tol = %.4f, |f32 model - truth| / tol = %.4f" % (what, par, g, o))
    RATIOS.append((what, par, g, o))
    helpers.TRUTH_LOG.append((os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], what + " (complex)", g, o))
    assert par <= 1.0, "%s: |gpu - f32 model| / tol = %.3g" % (what, par)
    assert g <= max(helpers.TRUTH_LIMIT, o), "%s: |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 composition's own %.3g)" % (
        what, g, helpers.TRUTH_LIMIT, o)
    return par, g, o


def cancelled_bound(cfg):
    """What a row whose composition is exactly 0 may hold: TRUTH_LIMIT (RTOL + ATOL_ROWMAX) eps_chain, eps_chain the epsilon the
    chain adds to its magnitudes (1e-5, the sim variant 1e-6) -- 5.05e-10 for the main variant."""
    eps_chain = 1e-6 if cfg.variant == VARIANT_SIM else 1e-5
    return helpers.TRUTH_LIMIT * (helpers.RTOL + helpers.ATOL_ROWMAX) * eps_chain


def check_rows(gpu, cfg, frames, yb, what, empty=(), cancelled=(), **kw):
    """check() with the rows of every frame in three classes.

    Rows in neither list: check()'s two assertions as they are -- parity with the float composition within the tolerance, and
    |gpu - truth| / tol <= max(TRUTH_LIMIT, the float composition's own ratio) -- over those rows.

    `empty` rows (degenerate_cases.exact_empty_rows): zeros before any rounding.  Every real and imaginary part equals 0; either
    sign of zero passes (values are compared, not bits).  The magnitude suite holds the same rows of the same arithmetic to
    float32(eps) bit for bit.

    `cancelled` rows (the no-fringe row on a clean background, the constant rows of degenerate_cases.dc_level_rows): the
    composition is exactly 0 in float and in double (tests/test_complex_cases.py), so RTOL |ref| + ATOL_ROWMAX rowmax|ref| is 0
    and cannot be used.  They are held to |gpu| <= TRUTH_LIMIT (RTOL + ATOL_ROWMAX) eps_chain (cancelled_bound).  That is what
    helpers.check_truth allows the magnitude image on the same row: there the truth is eps_chain in every bin, its tolerance
    RTOL eps_chain + ATOL_ROWMAX rowmax(eps_chain) = (RTOL + ATOL_ROWMAX) eps_chain, of which TRUTH_LIMIT is allowed, and the
    image's distance from it is ||gpu| + eps_chain - eps_chain| = |gpu|.  Nothing in it is a new number.

    Every figure is printed before anything is asserted; the call appends to helpers.TRUTH_LOG and RATIOS as check() does.
    Returns the three ratios of the rows in neither list (0 where there are none)."""
    gpu = np.asarray(gpu)
    assert gpu.dtype == np.complex64 and np.isfinite(gpu.view(np.float32)).all(), what + ": not finite complex64"
    H = gpu.shape[-2]
    empty, cancelled = sorted(set(empty)), sorted(set(cancelled))
    assert not set(empty) & set(cancelled) and all(0 <= r < H for r in empty + cancelled), (empty, cancelled)
    rows = [r for r in range(H) if r not in empty and r not in cancelled]
    par = g = o = 0.0
    if rows:
        ref = model(cfg, frames, yb, **kw)
        truth = model(cfg, frames, yb, truth=1, **kw)
        assert gpu.shape == ref.shape, (gpu.shape, ref.shape)
        par, g, o = ratio(gpu[:, rows], ref[:, rows]), ratio(gpu[:, rows], truth[:, rows]), ratio(ref[:, rows], truth[:, rows])
    bound = cancelled_bound(cfg)
    off = int(np.count_nonzero(gpu[:, empty])) if empty else 0
    left = float(np.abs(gpu[:, cancelled].astype(np.complex128)).max()) if cancelled else 0.0
    print("%s: |gpu - f32 model| / tol = %.4f, |gpu - truth| / tol = %.4f, |f32 model - truth| / tol = %.4f; empty rows %s: %d bins "
          "not 0; cancelled rows %s: max |gpu| = %.3g (bound %.3g)" % (what, par, g, o, empty, off, cancelled, left, bound))
    RATIOS.append((what, par, g, o))
    helpers.TRUTH_LOG.append((os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], what + " (complex)", g, o))
    assert par <= 1.0, "%s: |gpu - f32 model| / tol = %.3g" % (what, par)
    assert g <= max(helpers.TRUTH_LIMIT, o), "%s: |gpu - truth| / tol = %.3g exceeds max(%.2g, the f32 composition's own %.3g)" % (
        what, g, helpers.TRUTH_LIMIT, o)
    assert off == 0, "%s: %d real or imaginary parts of the empty rows %s are not 0" % (what, off, empty)
    assert left <= bound, "%s: the cancelled rows %s hold up to %.3g, beyond %.3g" % (what, cancelled, left, bound)
    return par, g, o
