"""BscanDark's lpfilter (BscanDark.cpp:119-167) restated in numpy, step by step, as the model of include/fdoct_lowpass.h.

For a row x[0 .. W-1] of doubles the reference does
  1. convertTo(CV_32F)
  2. dft(DFT_SCALE | DFT_COMPLEX_OUTPUT | DFT_ROWS):  F[k] = (1 / W) sum_n x[n] e^(-2 pi i k n / W)
  3. swaps the column halves [0, cx) and [cx, 2 cx), cx = W / 2 in integer division (an odd W keeps its last column in place)
  4. zeroes the shifted columns [0, dcl) and [dcr, dcr + dcl), dcl = W / 2 - W / 10, dcr = W / 2 + W / 10
  5. swaps the halves back
  6. dft(DFT_INVERSE | DFT_REAL_OUTPUT | DFT_ROWS), unscaled, which reads bins 0 .. W / 2 of its complex input as a
     conjugate-symmetric spectrum (the imaginary parts of bin 0 and, for an even W, of bin W / 2 do not enter)
  7. convertTo(CV_64F)

lpfilter_truth runs steps 2-6 in float64 / complex128 on actual arrays: the reference's mathematics.  lpfilter_f32 runs all
seven with float32 / complex64 transforms (numpy 2 transforms single precision in single): what a float transform such as
cv::dft's gives, up to the order of its butterflies.  lowpass_closed_form is the derivation the kernel evaluates;
tests/test_lowpass_model.py holds it against the literal steps."""
import numpy as np


def _swap_halves(F):
    cx = F.shape[1] // 2
    left = F[:, :cx].copy()
    F[:, :cx] = F[:, cx:2 * cx]
    F[:, cx:2 * cx] = left


def _literal(x, real, cplx):
    x = np.atleast_2d(np.asarray(x, np.float64))
    W = x.shape[1]
    F = (np.fft.fft(x.astype(real), axis=1) / real(W)).astype(cplx)        # steps 1, 2
    _swap_halves(F)                                                          # step 3
    dcl, dcr = W // 2 - W // 10, W // 2 + W // 10
    F[:, :dcl] = 0                                                           # step 4
    F[:, dcr:dcr + dcl] = 0
    _swap_halves(F)                                                          # step 5
    y = np.fft.irfft(F[:, :W // 2 + 1], n=W, axis=1).astype(real) * real(W)  # step 6 (irfft scales by 1 / W: undone)
    return y.astype(np.float64)                                              # step 7


def lpfilter_truth(x):
    """Steps 2-6 in float64 on (rows, W) doubles (one row: (1, W))."""
    return _literal(x, np.float64, np.complex128)


def lpfilter_f32(x):
    """Steps 1-7 with the transforms in float32."""
    return _literal(x, np.float32, np.complex64)


def lowpass_closed_form(x):
    """y[m] = Re F[0] + 2 sum_{k=1}^{f-1} Re(F[k] e^(+2 pi i k m / W)), f = W // 10, by direct sums in float64; W = 1, whose
    blanked ranges are empty, is its own result."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    W = x.shape[1]
    if W == 1:
        return x.copy()
    n = np.arange(W)
    y = np.zeros(x.shape)
    for k in range(W // 10):
        ph = np.exp(2j * np.pi * ((k * n) % W) / W)
        Fk = (x * ph.conj()).sum(axis=1) / W
        y += (1.0 if k == 0 else 2.0) * (Fk[:, None] * ph).real
    return y


def tolerance(truth):
    """The project's rule per element: 1e-4 |truth| + 1e-6 max over the row of |truth|."""
    truth = np.atleast_2d(truth)
    return 1e-4 * np.abs(truth) + 1e-6 * np.abs(truth).max(axis=1, keepdims=True)


def parity(got, x, truth=None):
    """(worst |got - truth| / tol, worst excess over the allowance) of the rule every GPU result is held to: on every element
    |got - truth| / tol <= max(0.5, |f32 model - truth| / tol).  A row whose truth is all zeros (W < 10) must be all zeros."""
    truth = lpfilter_truth(x) if truth is None else np.atleast_2d(truth)
    got = np.atleast_2d(got)
    assert got.shape == truth.shape
    tol = tolerance(truth)
    zero = tol == 0
    safe = np.where(zero, 1.0, tol)
    err = np.where(zero, np.where(got == 0, 0.0, np.inf), np.abs(got - truth) / safe)
    ref = np.where(zero, 0.0, np.abs(lpfilter_f32(x) - truth) / safe)
    return float(err.max()), float((err - np.maximum(0.5, ref)).max())
