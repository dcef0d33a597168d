"""CPU tests of tests/complex_model.py: the composition that specifies the complex A-scan is the oracle's own chain.  On every
shape the modulus of the float composition is the oracle's magI bit for bit -- so a kernel held to the composition is held to the
same numbers the magnitude tests hold it to, plus their phase -- and the truth composition's modulus is the truth magnitude to
1e-14 of the A-scan's peak (both are the same double operations; only the last square root differs, hypot against sqrt of the
sum of squares, an ulp of 1.1e-16 each)."""
import numpy as np
import pytest

import complex_model as cm
from fdoct_amd import Config, synth

H = 4
# (what, W, M, N, phase)
SHAPES = [
    ("128 -> 128", 128, 1, 128, False),
    ("128 -> 128, phase", 128, 1, 128, True),
    ("2048 -> 2048", 2048, 1, 2048, False),
    ("2048 -> 2048, phase", 2048, 1, 2048, True),
    ("200 x4 -> 2560", 200, 4, 2560, False),
    ("2048 -> 2002", 2048, 1, 2002, False),
    ("322 x4 -> 1288", 322, 4, 1288, False),
    ("64 -> 67", 64, 1, 67, False),
    ("200 x4 -> 2560, pi + dark + whole-frame normalisation", 200, 4, 2560, False),
]


def _case(what, W, M, N, phase):
    # numdisplaypoints = numfftpoints: every bin of the row is compared
    kw = {}
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=N, increasefftpointsmultiplier=M)
    if "normalisation" in what:
        cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=N, increasefftpointsmultiplier=M, donotnormalize=0)
        rng = np.random.default_rng(11)
        kw = dict(yp=rng.uniform(0.0, 0.02, (H, W)), yd=rng.uniform(90.0, 110.0, (H, W)))
    if phase:
        kw["phase"] = synth.dispersion_phase(N)
    frames = synth.make_frames(2, 2, W, H)
    yb = synth.make_background(W).astype(np.float64)
    if "normalisation" in what:
        yb = yb / 65535.0   # (the normalised frame lies in [0, 1])
    return cfg, frames, yb, kw


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_modulus_of_the_float_composition_is_the_oracles_magnitude_bit_for_bit(shape):
    cfg, frames, yb, kw = _case(*shape)
    X, mag = cm.model(cfg, frames, yb, want_mag=True, **kw)
    assert X.dtype == np.complex64 and mag.dtype == np.float32 and X.shape == mag.shape == (2, H, cfg.numfftpoints)
    re, im = X.real, X.imag
    mod = np.sqrt(re * re + im * im)   # main:1190 in float, as the oracle writes it
    assert mod.dtype == np.float32
    np.testing.assert_array_equal(mod.view(np.uint32), mag.view(np.uint32))
    assert mag.max() > 0 and np.abs(im).max() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_modulus_of_the_truth_composition_is_the_truth_magnitude(shape):
    cfg, frames, yb, kw = _case(*shape)
    X, mag = cm.model(cfg, frames, yb, truth=1, want_mag=True, **kw)
    assert X.dtype == np.complex128 and mag.dtype == np.float64
    assert (np.abs(np.abs(X) - mag) / mag.max(axis=-1, keepdims=True)).max() <= 1e-14
    # ... and the float composition is a small fraction of the tolerance from it (the inputs of the GPU tests are these frames)
    assert cm.ratio(cm.model(cfg, frames, yb, **kw), X) < 0.1
