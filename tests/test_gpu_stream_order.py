"""The stream-order contract of every entry point, on a busy stream ("Stream order"): calls of one handle run in call
order; a setter takes effect for later calls only; a call with a host-memory argument returns drained; set_stream orders the new
stream behind the old.  On an idle device all of this holds by timing alone -- a kernel on the wrong stream, a table overwritten under a
call still queued, finish in the right order anyway.  Here the caller's stream S is kept busy by a stall of known length
(tests/stream_stall.py) while the host enqueues behind it, so a violation changes a result.

The reference of every comparison is the quiet run: the same call sequence on a second handle of the same configuration with
torch.cuda.synchronize() between all steps.  The comparison is bit for bit (every stage here gives the same bits on a rerun).  Once per
kernel family the quiet chain result is also held to the oracle (helpers.check_mag), as tests/test_gpu_degenerate_inputs.py does:
two runs that agree on something wrong do not pass.

a. residency       inputs are filled on S behind the stall, outputs hold NaN poison; the call equals the quiet run only if all its
                   device work ran on the handle's stream.  Two controls leave the handle on its own stream and must NOT equal it.
b. setters         call A, a setter, call B, all behind the stall: A equals the quiet A under the old state, B the quiet B under the
                   new; the quiet distance between "A under the old state" and "A under the new" is printed and asserted to be
                   far more than a bit (set_staged and set_launch, which change no bit by design, are held to a distance of 0).
c. growth          call A, then a call B that outgrows a workspace A is using (tests/stream_cases.py: GROWTH), on a handle pair
                   that no other case uses, so that B does grow it.
d. stream switch   state accumulated on a stalled stream S1, set_stream(S2), the call that emits: against the NumPy models.  (Manual
                   averaging and the peak holds; a reference capture accumulates within one call, which returns drained, so it has
                   no state to carry across a switch.)
e. the rest        130 launches through the 64 ticket words of the workgroup-per-row kernel, close() with a call in flight, host-memory
                   calls on a handle whose caller's stream is stalled.

Every case that uses a stall asserts that the stall is still running when its call A has returned; an entry that hands a result back
in host memory returns drained by contract, and is held to that instead (the stall is over when it returns).  Handles are shared by
the cases of a configuration, put back into their start state by every case and warmed by one quiet call A before anything is
stalled, so that tables, run-time compiles and workspaces exist; they are closed when the module is done."""
import dataclasses
import time

import numpy as np
import pytest

import degenerate_cases as dg
import helpers
import manualavg_model
import roi_model
import stream_cases as sc
import stream_stall as ss
from fdoct_amd import Config, Reconstructor, capi, synth

pytestmark = pytest.mark.gpu

HXD, DXH = capi.LAYOUT_ROWMAJOR, capi.LAYOUT_TRANSPOSED
U8, U16, F64 = capi.DTYPE_U8, capi.DTYPE_U16, capi.DTYPE_F64
C0 = dg.C("plain", "clean")
FAR = 1e-3            # "far more than a bit": a relative distance of 1e-3 is 2^14 float ulps

ENQUEUE_MS = {}       # case -> warm host-side time of its call A with no stall in front: the smallest of three
ENQUEUE_ONCE_MS = {}  # ... of the calls A that keep state and are therefore timed once
CASE_MS = {}          # case -> wall time of its stalled run
DISTANCES = []        # (case, quiet distance between A under the old state and A under the new)


# ---- handles ------------------------------------------------------------------------------------------------------------------------------
class _Pool:
    def __init__(self):
        self.h = {}

    def get(self, key, make):
        if key not in self.h:
            self.h[key] = make()
        return self.h[key]

    def close(self):
        for r in self.h.values():
            try:
                r.set_stream(None)
            finally:
                r.close()
        self.h.clear()


POOL = _Pool()


@pytest.fixture(scope="module", autouse=True)
def _handles():
    import torch
    yield
    torch.cuda.synchronize()
    POOL.close()


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------
class _Bufs:
    """Device copies of a case's inputs (`src`, filled once), the inputs the calls read (`inp`) and their outputs (`out`), all as bytes."""

    def __init__(self, inputs, outputs):
        import torch
        self.src = {k: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda() for k, a in inputs.items()}
        self.inp = {k: torch.empty_like(t) for k, t in self.src.items()}
        self.meta = dict(outputs)
        self.out = {k: torch.empty(int(np.prod(shape)) * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
                    for k, (shape, dt) in outputs.items()}
        self.ptr = {k: t.data_ptr() for k, t in list(self.inp.items()) + list(self.out.items())}

    def poison(self):
        for t in self.inp.values():
            t.fill_(0xA5)
        for t in self.out.values():
            t.fill_(0xFF)          # floats: NaN

    def fill(self):
        for k, t in self.inp.items():
            t.copy_(self.src[k])

    def read(self):
        return {k: self.out[k].cpu().numpy().view(dt).reshape(shape).copy() for k, (shape, dt) in self.meta.items()}


class Case:
    """prep(rec): the start state.  steps: callables (rec, pointers) -> None or a host result; steps[0] is call A.  rearm(rec): what
    puts back the state the warm-up's call A changed.  finish(rec): host-side results read when everything has run.  drains: call A
    hands a result back in host memory.  setter: index of the setter among the steps (group b).  stateless: call A may be repeated."""

    def __init__(self, name, key, make, prep, inputs, outputs, steps, rearm=None, finish=None, drains=False, setter=None,
                 stateless=True, distance=None, check=None, main=None):
        self.main = main          # group b: the output of call A whose distance between the two states is reported
        self.name, self.key, self.make, self.prep, self.inputs, self.outputs, self.steps = name, key, make, prep, inputs, outputs, steps
        self.rearm, self.finish, self.drains, self.setter, self.stateless = rearm, finish, drains, setter, stateless
        self.distance, self.check = distance, check


def _sync():
    import torch
    torch.cuda.synchronize()


def _warm(case, rec, bufs):
    rec.set_stream(None)
    case.prep(rec)
    bufs.fill()
    _sync()
    case.steps[0](rec, bufs.ptr)
    _sync()
    if case.rearm:
        case.rearm(rec)
        _sync()


def _collect(case, rec, bufs, rets):
    out = bufs.read()
    for i, r in enumerate(rets):
        if r is not None:
            out["returned by step %d" % i] = np.asarray(r)
    if case.finish:
        for k, v in case.finish(rec).items():
            out[k] = np.asarray(v)
    return out


QUIET = {}


def run_quiet(case, state="old"):
    """The quiet run.  state 'new' (group b): the setter first, then call A alone -- A under the new state."""
    if (case.name, state) in QUIET:
        return QUIET[case.name, state]
    rec = POOL.get(case.key + " / quiet", case.make)
    bufs = _Bufs(case.inputs, case.outputs)
    _warm(case, rec, bufs)
    if state == "old" and case.stateless:
        ENQUEUE_MS[case.name] = ss.enqueue_ms(lambda: case.steps[0](rec, bufs.ptr), repeat=3)
    bufs.poison()
    bufs.fill()
    _sync()
    steps = case.steps if state == "old" else [case.steps[case.setter], case.steps[0]]
    rets = []
    for i, s in enumerate(steps):
        t0 = time.perf_counter()
        rets.append(s(rec, bufs.ptr))
        if state == "old" and i == 0 and not case.stateless:
            ENQUEUE_ONCE_MS[case.name] = (time.perf_counter() - t0) * 1e3
        _sync()
    if state == "new":
        rets = [rets[1]]
    out = _collect(case, rec, bufs, rets)
    if state == "old" and case.check:
        case.check(rec, out)
    QUIET[case.name, state] = out
    return out


def run_busy(case, handle_on_own_stream=False):
    """The same steps behind a stall on a caller's stream S, with the inputs filled on S.  handle_on_own_stream: the residency
    control -- the producer is on S, the handle is not."""
    import torch
    rec = POOL.get(case.key + " / busy", case.make)
    S = torch.cuda.Stream()
    bufs = _Bufs(case.inputs, case.outputs)
    t_case = time.perf_counter()
    try:
        _warm(case, rec, bufs)
        bufs.poison()
        _sync()
        if not handle_on_own_stream:
            rec.set_stream(S.cuda_stream)
        ev = ss.stall(S)
        with torch.cuda.stream(S):
            bufs.fill()
        rets = []
        for i, s in enumerate(case.steps):
            rets.append(s(rec, bufs.ptr))
            if i == 0 and not case.drains:
                ss.still_running(ev, case.name)
            if i == 0 and case.drains and not handle_on_own_stream:
                assert ev.query(), case.name + ": the call hands a result back in host memory and returned with the stream still busy"
        S.synchronize()
        rec.synchronize()
        return _collect(case, rec, bufs, rets)
    finally:
        S.synchronize()
        _sync()
        rec.set_stream(None)
        CASE_MS[case.name] = (time.perf_counter() - t_case) * 1e3


def differences(got, want):
    """Outputs that differ, as text; empty when everything is equal bit for bit."""
    bad = []
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(want):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            n = int((g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)).sum())
            bad.append("%s: %d of %d bytes differ" % (k, n, g.nbytes))
    return bad


def same(got, want, what):
    bad = differences(got, want)
    assert not bad, "%s differs from its reference: %s" % (what, "; ".join(bad))


def distance(a, b):
    """The largest elementwise |a - b| / max(|a|, |b|) over the common prefix of two outputs (0: the same values)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    n = min(a.size, b.size)
    a, b = a[:n].astype(np.float64), b[:n].astype(np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    d = np.abs(a - b)[ok] / np.maximum(np.maximum(np.abs(a), np.abs(b))[ok], 1e-300)
    return float(d.max()) if d.size else 0.0


# ---- the chain's calls ------------------------------------------------------------------------------------------------------------------------
def _frames(frame, n):
    """n distinct frames of one: the rows rolled by one more each."""
    return np.stack([np.roll(frame, k, axis=0) for k in range(n)])


class Chain:
    """process_device on a kernel family of tests/degenerate_cases.py: its handle, its start state and its calls."""

    def __init__(self, fam_name, dgcase=C0, cfg_over=None, extra=None, dtype=U16, raw=(1, 1), tag=""):
        self.fam, self.dgcase = dg.family(fam_name), dgcase
        self.i = dg.inputs(fam_name, dgcase)
        self.cfg = dataclasses.replace(self.i.cfg, **(cfg_over or {}))
        self.extra, self.dtype, self.raw = extra, dtype, raw
        self.key = "%s, %s%s" % (fam_name, dgcase.opt, tag)
        self.W, self.H, self.D = self.cfg.width, self.cfg.height, self.cfg.numdisplaypoints

    def make(self):
        return Reconstructor(dataclasses.replace(self.cfg))

    def reset(self, rec, yb=None):
        """Every setting back to the family's own: the handle is shared by the cases of its configuration."""
        rec.set_stream(None)
        rec.calibrate_clear()
        rec.set_frontend(0, 1, 1)
        rec.set_colour_input(-1)
        rec.set_raw_magnitudes(False)
        rec.set_averages(self.cfg.averages)
        rec.set_bandpass(False)
        rec.set_precise_division(True)
        rec.set_jit(True)
        rec.set_launch(0, 0)
        rec.set_window(None)
        rec.set_lambda_range(self.cfg.lambdamin, self.cfg.lambdamax)
        rec.set_dispersion_phase(None)
        rec.set_staged(False)
        rec.set_plan(-1, self.fam.setup == "any-option")
        rec.set_staged(self.fam.setup == "staged")
        rec.set_pi_frame(None)
        rec.set_dark(None)
        rec.set_background(self.i.yb if yb is None else yb)
        if self.extra:
            self.extra(rec)

    def frames(self, n):
        f = self.i.frames[0]
        if self.raw != (1, 1):     # raw camera frames for a front end that bins: every pixel repeated
            f = np.repeat(np.repeat(f, self.raw[1], axis=0), self.raw[0], axis=1)
        if self.dtype == F64:
            f = f.astype(np.float64) / 7.0 + 0.25
        return _frames(f, n)

    def out_shape(self, n, layout, averages=None):
        g = n // (averages or self.cfg.averages)
        return (g, self.D, self.H) if layout == DXH else (g, self.H, self.D)

    def call(self, n, x="x", mag="mag", db="db", layout=HXD, dtype=None):
        dt = self.dtype if dtype is None else dtype
        return lambda rec, p: rec.process_device(p[x], dt, n, 0, p.get(mag), p.get(db), layout)

    def case(self, name, n=1, layout=HXD, want_db=True, check=None):
        outs = {"mag": (self.out_shape(n, layout), np.float32)}
        if want_db:
            outs["db"] = (self.out_shape(n, layout), np.float32)
        return Case(name, self.key, self.make, self.reset, {"x": self.frames(n)}, outs, [self.call(n, layout=layout)], check=check)


def _oracle_check(chain, layout):
    """The quiet result against the oracle, and the kernel family the call took."""
    def check(rec, out):
        want_kernel = dg.expected_kernel(chain.fam, chain.dgcase)
        if layout == chain.fam.layout:
            assert rec.last_kernel() == want_kernel, (chain.fam.name, rec.last_kernel(), want_kernel, rec.jit_note())
        mag = out["mag"] if layout == HXD else np.transpose(out["mag"], (0, 2, 1))
        mag_o = dg.reference(chain.fam.name, chain.dgcase)[0]
        worst = helpers.check_mag(mag, mag_o, "%s, quiet run" % chain.fam.name)
        print("%s, layout %d: quiet run against the oracle, worst error / tolerance %.3g" % (chain.fam.name, layout, worst))
    return check


RESIDENCY = {}       # name -> () -> Case
SETTERS = {}
GROWTH = {}


def _add(reg, name, build):
    assert name not in reg, name
    reg[name] = build


def _named(group, name, reg):
    """The case of a registry under a name of its own: the quiet runs are cached by it."""
    case = reg[name]()
    case.name = "%s. %s" % (group, name)
    return case


def _family_layouts(fam):
    if fam.setup == "staged":
        return [HXD]
    return [fam.layout, DXH if fam.layout == HXD else HXD]


for _fam in dg.FAMILIES:
    for _lay in _family_layouts(_fam):
        def _build(fam=_fam, lay=_lay):
            ch = Chain(fam.name)
            return ch.case("process_device, %s, layout %d" % (fam.name, lay), layout=lay, check=_oracle_check(ch, lay))
        _add(RESIDENCY, "process_device: %s, %s" % (_fam.name, "D x H" if _lay == DXH else "H x D"), _build)

GEN = "workgroup-per-row, 2048 -> 2002"
FAST = "fused fast path, 1024-point plan"
WAVE = "wave-per-row, 160 x 4"
JIT = "wave-per-row, run-time compiled, 200 x 4"
BLUESTEIN = "workgroup-per-row, Bluestein, 322 x 4"
U8FAM = "wave-per-row, 640 x 1, 8-bit"


# the chain's front passes, as residency cases and (two sizes) as growth pairs
def _front_chains():
    return {
        "movavgn 3 on u16 frames": lambda: Chain(GEN, cfg_over=dict(movavgn=3), tag=", movavgn 3"),
        "f64 frames, the split planes": lambda: Chain(GEN, dtype=F64, tag=", f64"),
        "the sim variant's gather, averages 2": lambda: Chain(GEN, dg.C("sim", "clean"), cfg_over=dict(averages=2), tag=", averages 2"),
        "whole-frame normalisation": lambda: Chain(FAST, dg.C("whole", "dead")),
        "set_frontend(3, 1, 1)": lambda: Chain(GEN, extra=lambda r: r.set_frontend(3, 1, 1), tag=", median 3"),
        "set_frontend(0, 2, 2)": lambda: Chain(GEN, extra=lambda r: r.set_frontend(0, 2, 2), raw=(2, 2), tag=", binning 2 x 2"),
        "set_frontend(3, 2, 2)": lambda: Chain(GEN, extra=lambda r: r.set_frontend(3, 2, 2), raw=(2, 2), tag=", median 3, binning 2 x 2"),
        "D x H through the transpose pass": lambda: Chain(GEN),
        "staged mode's k-linear rows": lambda: Chain("fused, staged"),
        "the long-row path's chunk": lambda: Chain("long rows, 2048 x 8"),
    }


for _what in ("movavgn 3 on u16 frames", "f64 frames, the split planes", "the sim variant's gather, averages 2",
              "whole-frame normalisation", "set_frontend(3, 1, 1)", "set_frontend(0, 2, 2)", "set_frontend(3, 2, 2)"):
    def _build(what=_what):
        ch = _front_chains()[what]()
        return ch.case("process_device, %s" % what, n=ch.cfg.averages)
    _add(RESIDENCY, "process_device: front pass, %s" % _what, _build)


def _growth_key(key, g):
    """A growth case has a handle pair of its own: Buffer::reserve only grows, so on a handle other cases have used the larger
    call may find its workspace large enough already and free nothing.  Here the only call before B is A (the warm-up's and the
    case's), and stream_cases.GROWTH holds B's need above A's."""
    return "%s, growth of %s" % (key, g.workspace)


def _chain_growth(what, layout=HXD):
    def build():
        g = sc.GROWTH[[x.site for x in sc.GROWTH].index(what)]
        ch = _front_chains()[what]()
        na, nb = g.small["nframes"], g.large["nframes"]
        outs = {"mag_a": (ch.out_shape(na, layout), np.float32), "db_a": (ch.out_shape(na, layout), np.float32),
                "mag_b": (ch.out_shape(nb, layout), np.float32), "db_b": (ch.out_shape(nb, layout), np.float32)}
        steps = [ch.call(na, "xa", "mag_a", "db_a", layout), ch.call(nb, "xb", "mag_b", "db_b", layout)]
        return Case("growth of %s" % g.workspace, _growth_key(ch.key, g), ch.make, ch.reset, {"xa": ch.frames(na), "xb": ch.frames(nb)[::-1]}, outs, steps)
    return build


# ---- the side stages (the shapes of tests/test_gpu_staging.py) ---------------------------------------------------------------------
SW, SH, SN, SD = (sc.SIDE[k] for k in "WHND")
SIDE_KEY = "side stages, 64 x 8"


def _side_make():
    rec = Reconstructor(Config(width=SW, height=SH, numfftpoints=SN, numdisplaypoints=SD))
    rec.set_background(synth.make_background(SW))
    return rec


def _side_prep(rec):
    rec.set_stream(None)
    rec.set_colormap(None)


def _side(name, inputs, outputs, steps, prep=None, **kw):
    def full_prep(rec):
        _side_prep(rec)
        if prep:
            prep(rec)
    return Case(name, SIDE_KEY, _side_make, full_prep, inputs, outputs, steps, **kw)


def _db_images(n, depths, layout, seed):
    a = np.random.default_rng(seed).uniform(-60.0, 10.0, (n, depths, SH)).astype(np.float32)
    return np.ascontiguousarray(a if layout == DXH else np.transpose(a, (0, 2, 1)))


def _u16_frames(n, seed=10):
    return np.random.default_rng(seed + n).integers(0, 4096, (n, SH, SW)).astype(np.uint16)


def _linear_images(n, seed):
    return np.random.default_rng(seed).uniform(0.5, 50.0, (n, SH, SD)).astype(np.float32)      # row-major: (n, ascans, depths)


def _side_ascan_minmax():
    n = 3
    return _side("ascan_minmax_device", {"a": _db_images(n, SD, HXD, 1)}, {"lo": ((n,), np.float32), "hi": ((n,), np.float32)},
                 [lambda r, p: r.ascan_minmax_device(p["a"], n, SD, SH, 3, p["lo"], p["hi"], HXD)])


def _side_roi_mean():
    n = 3
    return _side("roi_mean_device", {"a": _db_images(n, SD, DXH, 2)}, {"out": ((n,), np.float64)},
                 [lambda r, p: r.roi_mean_device(p["a"], n, SD, SH, 2, 1, 3, p["out"], DXH)])


ROI_1, ROI_2 = (1, 1, 4, 3, 2), (2, 3, 5, 6, 6)     # x, y, w, h, ascanat: different widths, so that the column holds are reallocated


def _holds(slots):
    def finish(rec):
        out = {}
        for s in slots:
            cols, amax, count = rec.peakhold_values(s)
            out["slot %d columns" % s], out["slot %d scalar and count" % s] = cols, np.array([amax, count], np.float64)
        return out
    return finish


def _roi_start(rec):
    rec.set_peakhold_roi(*ROI_1)
    for s in (1, 2):
        rec.clear_peakhold(s)


def _side_peakhold():
    n = 3
    return _side("peakhold_device", {"a": _db_images(n, SD, HXD, 3)}, {}, [lambda r, p: r.peakhold_device(2, p["a"], n, SD, SH, HXD)],
                 prep=_roi_start, rearm=_roi_start, finish=_holds((2,)), stateless=False)


def _side_clear_peakhold():
    """A fold, the clear, a second fold: the slot holds the second fold alone only if the clear's memsets ran between them."""
    n = 2
    steps = [lambda r, p: r.peakhold_device(2, p["a"], n, SD, SH, HXD), lambda r, p: r.clear_peakhold(2),
             lambda r, p: r.peakhold_device(2, p["b"], n, SD, SH, HXD)]
    return _side("clear_peakhold", {"a": _db_images(n, SD, HXD, 4) + 30.0, "b": _db_images(n, SD, HXD, 5)}, {}, steps, prep=_roi_start,
                 rearm=_roi_start, finish=_holds((2,)), stateless=False)


def _side_set_peakhold_roi():
    """A fold into slot 1 under the first ROI, a second ROI of another width (the column holds are reallocated and reset, the scalar
    holds stay), a fold into slot 2: slot 1's scalar is the first fold's under the first ROI, slot 2 holds the second fold alone."""
    n = 2
    steps = [lambda r, p: r.peakhold_device(1, p["a"], n, SD, SH, HXD), lambda r, p: r.set_peakhold_roi(*ROI_2),
             lambda r, p: r.peakhold_device(2, p["b"], n, SD, SH, HXD)]
    # (values above 0, where the scalar holds start: the first fold's hold is then a maximum of its own ROI's samples)
    return _side("set_peakhold_roi", {"a": _db_images(n, SD, HXD, 6) + 60.0, "b": _db_images(n, SD, HXD, 7) + 60.0}, {}, steps, prep=_roi_start,
                 rearm=_roi_start, finish=_holds((1, 2)), stateless=False, setter=1, distance=FAR, main="slot 1 scalar and count")


def _side_frame_minmax(n=3, name="frame_minmax_device", sfx=""):
    return ({"f" + sfx: _u16_frames(n)}, {"lo" + sfx: ((n,), np.float64), "hi" + sfx: ((n,), np.float64)},
            lambda r, p: r.frame_minmax_device(p["f" + sfx], U16, n, 0, p["lo" + sfx], p["hi" + sfx]))


def _side_capture_reference():
    n = 3
    return _side("capture_reference_device", {"f": _u16_frames(n)}, {},
                 [lambda r, p: r.capture_reference_device(capi.REF_NONE, p["f"], U16, n, 0, out=True)], drains=True)


def _side_calibrate_capture():
    n = 3
    return _side("calibrate_capture_device", {"f": _u16_frames(n, 20)}, {},
                 [lambda r, p: r.calibrate_capture_device(capi.CAL_REFERENCE, p["f"], U16, n, 0, out=True)], drains=True,
                 prep=lambda r: r.calibrate_clear())


def _lowpass_io(rows, width, sfx=""):
    a = np.random.default_rng(20 + rows).uniform(-1.0, 1.0, (rows, width))
    return ({"a" + sfx: a}, {"out" + sfx: ((rows, width), np.float64)},
            lambda r, p: r.lowpass_rows_device(p["a" + sfx], rows, width, 0, p["out" + sfx]))


def _normalize_io(rows, sfx=""):
    a = np.random.default_rng(30 + rows).uniform(-3.0, 9.0, (rows, SW))
    return ({"a" + sfx: a}, {"out" + sfx: ((rows, SW), np.float64)},
            lambda r, p: r.normalize_rows_minmax_device(p["a" + sfx], rows, SW, 0, 0.0001, 1.0, True, p["out" + sfx]))


def _bscan_bin_io(factor, sfx="", seed=30):
    n = 2
    return ({"a" + sfx: _linear_images(n, seed)}, {"lin" + sfx: ((n, SH, SD), np.float32), "db" + sfx: ((n, SH, SD), np.float32)},
            lambda r, p: r.bscan_bin_device(p["a" + sfx], n, SD, SH, factor, factor, p["lin" + sfx], p["db" + sfx]))


def _display_io(n, sfx="", seed=40):
    a = np.random.default_rng(seed).uniform(-70.0, 5.0, (n, 6, 7)).astype(np.float32)
    return ({"a" + sfx: a}, {"gray" + sfx: ((n, 6, 7), np.uint8), "bgr" + sfx: ((n, 6, 7, 3), np.uint8)},
            lambda r, p: r.display_device(p["a" + sfx], n, 6, 7, p["gray" + sfx], p["bgr" + sfx], clampupper=True))


def _side_lockin():
    b, j = _linear_images(2, 50), _linear_images(1, 51)[0]
    return _side("lockin_db_device", {"b": b, "j": j}, {"out": (b.shape, np.float32)},
                 [lambda r, p: r.lockin_db_device(p["b"], p["j"], 2, j.size, p["out"])])


def _colour_io(n, channelnum, sfx=""):
    bgr = np.random.default_rng(70 + n).integers(0, 256, (n, SH, SW, 3)).astype(np.uint8)
    return ({"bgr" + sfx: bgr}, {"out" + sfx: ((n, SH, SW), np.float64 if channelnum == 3 else np.uint8)},
            lambda r, p: r.colour_extract_device(p["bgr" + sfx], n, SW, SH, 3 * SW, channelnum, p["out" + sfx]))


def _saveframes_io(n, averages, sfx=""):
    g = n // averages if averages else 0
    outs = {"gray" + sfx: ((n, SD, SH), np.uint8)}
    if g:
        outs.update({"b" + sfx: ((g, SD, SH), np.float32), "db" + sfx: ((g, SD, SH), np.float32)})
    return ({"a" + sfx: _linear_images(n, 80 + n)}, outs,
            lambda r, p: r.saveframes_device(p["a" + sfx], n, SD, SH, p["gray" + sfx], averages, p.get("b" + sfx), p.get("db" + sfx), HXD, DXH))


def _doppler_io(n, bulk, sfx=""):
    rng = np.random.default_rng(90 + n)
    X = (rng.standard_normal((n, SH, SD)) + 1j * rng.standard_normal((n, SH, SD))).astype(np.complex64)
    shp = (n, SH - 1, SD)
    return ({"x" + sfx: X}, {"phase" + sfx: (shp, np.float32), "corr" + sfx: (shp, np.complex64), "power" + sfx: (shp, np.float32)},
            lambda r, p: r.doppler_device(p["x" + sfx], n, SH, SD, capi.DOPPLER_ASCANS, 1, p["phase" + sfx], p["corr" + sfx], p["power" + sfx],
                                          win=(2, 2), bulk=bulk))


COUNT = SH * SD


def _mavg_images(n, seed):
    return np.random.default_rng(seed).uniform(0.5, 50.0, (n, SH, SD)).astype(np.float32)


def _side_manualavg_add():
    begin = lambda r: r.manualavg_begin(2, COUNT, capi.MANUALAVG_KEEP_ALL)      # noqa: E731
    return _side("manualavg_add_device", {"a": _mavg_images(2, 60)}, {"mean": ((1, SH, SD), np.float32), "db": ((1, SH, SD), np.float32)},
                 [lambda r, p: r.manualavg_add_device(p["a"], 2, p["mean"], p["db"], 1)], prep=begin, rearm=begin, stateless=False)


def _side_manualavg_begin():
    """Three images into an accumulator of three (emits their mean), a new accumulator of two, two images (emits): the first call's
    emitted images keep their bits, the second mean holds the two alone.  (Under the new state call A emits the mean of its first
    two images: the distance between the two states.)"""
    begin = lambda r: r.manualavg_begin(3, COUNT, capi.MANUALAVG_KEEP_ALL)      # noqa: E731
    outs = {k: ((1, SH, SD), np.float32) for k in ("mean_a", "db_a", "mean_b", "db_b")}
    steps = [lambda r, p: r.manualavg_add_device(p["a"], 3, p["mean_a"], p["db_a"], 1),
             lambda r, p: r.manualavg_begin(2, COUNT, capi.MANUALAVG_KEEP_ALL),
             lambda r, p: r.manualavg_add_device(p["b"], 2, p["mean_b"], p["db_b"], 1)]
    return _side("manualavg_begin", {"a": _mavg_images(3, 61), "b": _mavg_images(2, 62)}, outs, steps, prep=begin, rearm=begin,
                 stateless=False, setter=1, distance=FAR, main="mean_a")


def _side_from(name, io, **kw):
    def build():
        inputs, outputs, step = io()
        return _side(name, inputs, outputs, [step], **kw)
    return build


_add(RESIDENCY, "ascan_minmax_device", _side_ascan_minmax)
_add(RESIDENCY, "roi_mean_device", _side_roi_mean)
_add(RESIDENCY, "peakhold_device", _side_peakhold)
_add(RESIDENCY, "clear_peakhold", _side_clear_peakhold)
_add(RESIDENCY, "set_peakhold_roi", _side_set_peakhold_roi)
_add(RESIDENCY, "frame_minmax_device", _side_from("frame_minmax_device", _side_frame_minmax))
_add(RESIDENCY, "capture_reference_device", _side_capture_reference)
_add(RESIDENCY, "calibrate_capture_device", _side_calibrate_capture)
_add(RESIDENCY, "lowpass_rows_device", _side_from("lowpass_rows_device", lambda: _lowpass_io(8, 64)))
_add(RESIDENCY, "normalize_rows_minmax_device", _side_from("normalize_rows_minmax_device", lambda: _normalize_io(8)))
_add(RESIDENCY, "bscan_bin_device", _side_from("bscan_bin_device", lambda: _bscan_bin_io(2)))
_add(RESIDENCY, "display_device", _side_from("display_device", lambda: _display_io(2)))
_add(RESIDENCY, "lockin_db_device", _side_lockin)
_add(RESIDENCY, "colour_extract_device", _side_from("colour_extract_device", lambda: _colour_io(2, 1)))
_add(RESIDENCY, "saveframes_device: pictures and fold", _side_from("saveframes_device", lambda: _saveframes_io(2, 2)))
_add(RESIDENCY, "doppler_device: no bulk", _side_from("doppler_device", lambda: _doppler_io(2, None)))
_add(RESIDENCY, "doppler_device: bulk", _side_from("doppler_device, bulk", lambda: _doppler_io(2, True)))
_add(RESIDENCY, "manualavg_add_device", _side_manualavg_add)
_add(RESIDENCY, "manualavg_begin", _side_manualavg_begin)


def _side_frontend():
    """fdoct_frontend takes host memory only: on a handle whose caller's stream is stalled it returns drained, with the quiet result."""
    raw = np.random.default_rng(60).integers(0, 4096, (1, 16, 128)).astype(np.uint16)
    return _side("frontend", {}, {}, [lambda r, p: r.frontend(raw, 3, 2, 2)], drains=True)


_add(RESIDENCY, "frontend", _side_frontend)


def _complex_case(layout):
    def build():
        ch = Chain(GEN)
        n = 2
        shp = (n, ch.D, ch.H) if layout == DXH else (n, ch.H, ch.D)
        return Case("process_complex_device, layout %d" % layout, ch.key, ch.make, ch.reset, {"x": ch.frames(n)}, {"cx": (shp, np.complex64)},
                    [lambda r, p: r.process_complex_device(p["x"], U16, n, 0, p["cx"], layout)])
    return build


_add(RESIDENCY, "process_complex_device: H x D", _complex_case(HXD))
_add(RESIDENCY, "process_complex_device: D x H", _complex_case(DXH))


def _process_doppler_case():
    ch = Chain(GEN)
    n = 2
    shp = (n, ch.H - 1, ch.D)
    outs = {"phase": (shp, np.float32), "corr": (shp, np.complex64), "power": (shp, np.float32)}
    return Case("process_doppler_device", ch.key, ch.make, ch.reset, {"x": ch.frames(n)}, outs,
                [lambda r, p: r.process_doppler_device(p["x"], U16, n, 0, capi.DOPPLER_ASCANS, 1, p["phase"], p["corr"], p["power"],
                                                       win=(2, 2), bulk=True)])


_add(RESIDENCY, "process_doppler_device", _process_doppler_case)


# ---- a. residency ------------------------------------------------------------------------------------------------------------------------
def test_the_stall_makes_a_violation_visible():
    """Torch alone, no library call: a copy queued behind the stall reads what another stream wrote in the meantime.  A plain data race
    on valid memory; nothing faults."""
    import torch
    S, other = torch.cuda.Stream(), torch.cuda.Stream()
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    out = torch.full((4096,), -1.0, dtype=torch.float32, device="cuda")
    new = torch.arange(4096, dtype=torch.float32, device="cuda") + 1.0
    torch.cuda.synchronize()
    try:
        ev = ss.stall(S)
        with torch.cuda.stream(S):
            out.copy_(buf)
        ss.still_running(ev, "teeth check")
        with torch.cuda.stream(other):
            buf.copy_(new)
        other.synchronize()
        ss.still_running(ev, "teeth check, after the overwrite")
        S.synchronize()
        assert torch.equal(out, new), "the copy behind the stall did not see the later write: the stall orders nothing"
    finally:
        S.synchronize()
        other.synchronize()
    cal = ss.calibration()
    print("stall: %s, %.0f per ms, a 10 ms stall measured %.2f ms; STALL_MS = %g" % (cal["mode"], cal["per_ms"], cal["check_ms"], ss.STALL_MS))
    assert 10.0 <= ss.STALL_MS <= 100.0


def test_the_catalogue_has_a_case_for_every_name():
    covered = {n.split(":")[0] for n in RESIDENCY}
    assert sorted(covered) == sorted(sc.ENTRIES), (sorted(set(sc.ENTRIES) - covered), sorted(covered - set(sc.ENTRIES)))
    covered = {n.split(" ")[0].rstrip(":") for n in SETTERS}
    assert sorted(covered) == sorted(sc.SETTERS), (sorted(set(sc.SETTERS) - covered), sorted(covered - set(sc.SETTERS)))
    assert sorted(GROWTH) == sorted(sc.GROWTH_IDS)
    for n in sc.DRAINING_ENTRIES:
        assert RESIDENCY[n]().drains, n


@pytest.mark.parametrize("name", list(RESIDENCY))
def test_every_entry_does_its_device_work_on_the_handles_stream(name):
    case = _named("a", name, RESIDENCY)
    want = run_quiet(case)
    same(run_busy(case), want, name)


@pytest.mark.parametrize("name", ["process_device: %s, H x D" % GEN, "saveframes_device: pictures and fold"])
def test_residency_control_a_handle_left_on_its_own_stream_consumes_poison(name):
    """The same call with the producer on the stalled stream and the handle on its own: the result must NOT equal the quiet run.
    This is what the comparison of the test above looks like when it fails."""
    case = _named("a", name, RESIDENCY)
    want = run_quiet(case)
    bad = differences(run_busy(case, handle_on_own_stream=True), want)
    print("%s, handle on its own stream: %s" % (name, "; ".join(bad)))
    assert bad, name + ": a call that cannot have seen its inputs equals the quiet run"


# ---- b. a state change does not reach back -----------------------------------------------------------------------------------------------------
def _setter_case(name, chain, old, new, n=1, n_b=None, layout=HXD, want_db=True, start_yb=None, averages_b=None, dist=FAR, check_b=None):
    """call A, new(rec), call B on one chain handle; old(rec) belongs to the start state."""
    n_b = n if n_b is None else n_b

    def prep(rec):
        chain.reset(rec, start_yb)
        if old:
            old(rec)
    outs = {"mag_a": (chain.out_shape(n, layout), np.float32), "mag_b": (chain.out_shape(n_b, layout, averages_b), np.float32)}
    if want_db:
        outs.update({"db_a": (chain.out_shape(n, layout), np.float32), "db_b": (chain.out_shape(n_b, layout, averages_b), np.float32)})
    steps = [chain.call(n, "x", "mag_a", "db_a", layout), lambda rec, p: new(rec), chain.call(n_b, "x", "mag_b", "db_b", layout)]
    return Case(name, chain.key, chain.make, prep, {"x": chain.frames(max(n, n_b))}, outs, steps, setter=1, distance=dist, check=check_b)


def _table_states(chain, start_kind):
    """name -> (old, new, background the handle starts with) of the table setters on one chain."""
    W, H, top = chain.W, chain.H, 65535
    row = dg.background("clean", W, H, top)
    row2 = np.ascontiguousarray(row[::-1]) * 0.5 + 100.0
    full = dg.background("full", W, H, top)
    start = full if start_kind == "full" else row
    frame = chain.i.frames[0]
    yp = 0.5 * frame.astype(np.float64)
    yd = dg.dark_frame(frame, top)
    window = np.linspace(0.2, 1.0, W) ** 2
    phase = synth.dispersion_phase(chain.cfg.numfftpoints)
    lo, hi = chain.cfg.lambdamin, chain.cfg.lambdamax
    narrow = (lo + 0.2 * (hi - lo), hi - 0.1 * (hi - lo))

    def reversed_table(rec):
        idx, frac = rec.get_resample_table()
        rec.set_resample_table(idx[::-1], frac[::-1])

    return {
        "set_background [1-row to 1-row]": (None, lambda r: r.set_background(row2), row),
        "set_background [1-row to H-row]": (None, lambda r: r.set_background(full), row),
        "set_background [H-row to 1-row]": (None, lambda r: r.set_background(row2), full),
        "set_pi_frame [set]": (None, lambda r: r.set_pi_frame(yp), start),
        "set_pi_frame [cleared]": (lambda r: r.set_pi_frame(yp), lambda r: r.set_pi_frame(None), start),
        "set_dark [set]": (None, lambda r: r.set_dark(yd), start),
        "set_dark [cleared]": (lambda r: r.set_dark(yd), lambda r: r.set_dark(None), start),
        "set_window": (None, lambda r: r.set_window(window), start),
        "set_resample_table": (None, reversed_table, start),
        "set_lambda_range": (None, lambda r: r.set_lambda_range(*narrow), start),
        "set_dispersion_phase [on]": (None, lambda r: r.set_dispersion_phase(phase), start),
        "set_dispersion_phase [off]": (lambda r: r.set_dispersion_phase(phase), lambda r: r.set_dispersion_phase(None), start),
    }


_TABLE_STATE_NAMES = ["set_background [1-row to 1-row]", "set_background [1-row to H-row]", "set_background [H-row to 1-row]",
                      "set_pi_frame [set]", "set_pi_frame [cleared]", "set_dark [set]", "set_dark [cleared]", "set_window",
                      "set_resample_table", "set_lambda_range", "set_dispersion_phase [on]", "set_dispersion_phase [off]"]
for _set, (_famname, _kind) in sc.TABLE_SETS.items():
    for _state in _TABLE_STATE_NAMES:
        def _build(famname=_famname, kind=_kind, state=_state, tset=_set):
            ch = Chain(famname)
            old, new, yb = _table_states(ch, kind)[state]
            return _setter_case("%s on %s" % (state, tset), ch, old, new, start_yb=yb)
        _add(SETTERS, "%s on %s" % (_state, _set), _build)


def _kernel_after_b(want):
    def check(rec, out):
        assert rec.last_kernel() == want, (rec.last_kernel(), want, rec.jit_note())
    return check


def _other_setters():
    yield "set_averages", lambda: _setter_case("set_averages", Chain(FAST), None, lambda r: r.set_averages(2), n=2, averages_b=2)
    yield "set_bandpass", lambda: _setter_case("set_bandpass", Chain(BLUESTEIN), None, lambda r: r.set_bandpass(True))
    # the next three change which kernel computes the same chain: the 11 rows of tests/degenerate_cases.py hold rows that are empty
    # but for a cancelled DC level, where a second word of 1 / background or another order of sums shows far above FAR
    yield "set_precise_division", lambda: _setter_case("set_precise_division", Chain(FAST), None, lambda r: r.set_precise_division(False))
    yield "set_plan (-1, True)", lambda: _setter_case("set_plan", Chain(FAST), None, lambda r: r.set_plan(-1, True),
                                                        check_b=_kernel_after_b(capi.KERNEL_FUSED))
    yield "set_jit", lambda: _setter_case("set_jit", Chain(JIT), None, lambda r: r.set_jit(False), check_b=_kernel_after_b(capi.KERNEL_GENERIC))
    # ... and these two leave every bit as it is, by design (staged mode equals the fused chain, one workgroup the whole grid: held
    # bit for bit by tests/test_gpu_degenerate_inputs.py and tests/test_gpu_parity.py).  A reach-back into call A cannot show in its
    # result, so it is not looked for there: the distance is held to 0 -- a change that makes the two states differ turns that
    # assertion on -- and what can be held is, that each call equals its quiet run and call B took the kernel the new state names
    yield "set_staged", lambda: _setter_case("set_staged", Chain(FAST), None, lambda r: r.set_staged(True), dist=0,
                                              check_b=_kernel_after_b(capi.KERNEL_FUSED_STAGED))
    yield "set_launch", lambda: _setter_case("set_launch", Chain(FAST), None, lambda r: r.set_launch(0, 1), dist=0,
                                              check_b=_kernel_after_b(capi.KERNEL_FUSED))
    yield "set_frontend", lambda: _setter_case("set_frontend", Chain(GEN), lambda r: r.set_frontend(3, 1, 1), lambda r: r.set_frontend(0, 1, 1))
    yield "set_raw_magnitudes", lambda: _setter_case("set_raw_magnitudes", Chain(GEN), None, lambda r: r.set_raw_magnitudes(True), want_db=False)
    yield "set_colour_input", _colour_input_case
    yield "import_state", _import_state_case
    yield "capture_reference_device (role background)", _capture_background_case
    yield "calibrate_compose", _calibrate_compose_case


def _colour_input_case():
    """Channel 0, then channel 2, of the same B,G,R frames."""
    ch = Chain(U8FAM, dg.C("plain", "clean", bits=8), dtype=U8)
    mono = ch.i.frames[0]
    bgr = np.stack([mono, np.roll(mono, 3, axis=0), (mono // 2 + 17).astype(np.uint8)], axis=-1)[None]
    case = _setter_case("set_colour_input", ch, lambda r: r.set_colour_input(0), lambda r: r.set_colour_input(2))
    case.inputs = {"x": bgr}
    return case


def _import_state_case():
    ch = Chain(FAST)
    row2 = np.ascontiguousarray(dg.background("clean", ch.W, ch.H, 65535)[::-1]) * 0.5 + 100.0
    blob = {}

    def old(rec):        # the blob of another background and window, made on the handle itself before anything is stalled
        rec.set_background(row2)
        rec.set_window(synth.hann_window(ch.W))
        blob["b"] = rec.export_state()
        ch.reset(rec)
    return _setter_case("import_state", ch, old, lambda r: r.import_state(blob["b"]))


def _capture_background_case():
    """The b key on device frames between two calls: the capture returns drained, the call behind it divides by the captured mean."""
    ch = Chain(FAST)
    case = _setter_case("capture_reference_device", ch, None, None)
    cap = _frames(np.roll(ch.i.frames[0], 5, axis=0), 2)
    case.inputs["cap"] = cap
    case.steps[1] = lambda rec, p: rec.capture_reference_device(capi.REF_BACKGROUND, p["cap"], U16, 2, 0)
    return case


def _calibrate_compose_case():
    """BscanDark's composition from three held captures becomes the background between two calls."""
    ch = Chain(FAST)
    f = ch.i.frames[0]
    dark = (f // 100)[None]
    ref, sample = _frames(np.roll(f, 2, axis=0), 2), _frames(np.roll(f, 7, axis=0), 2)

    def old(rec):
        rec.calibrate_capture(capi.CAL_DARK, dark)
        rec.calibrate_capture(capi.CAL_REFERENCE, ref)
        rec.calibrate_capture(capi.CAL_SAMPLE, sample)
    return _setter_case("calibrate_compose", ch, old, lambda r: r.calibrate_compose())


for _name, _build in _other_setters():
    _add(SETTERS, _name, _build)


def _colormap_case():
    inputs, outputs, step_a = _display_io(2, "_a", 41)
    i2, o2, step_b = _display_io(2, "_b", 42)
    inputs.update(i2), outputs.update(o2)
    lut = np.ascontiguousarray(capi.build_colormap_jet()[::-1])
    return _side("set_colormap", inputs, outputs, [step_a, lambda r, p: r.set_colormap(lut), step_b], setter=1, distance=FAR, main="bgr_a")


def _bscan_bin_factors_case():
    """Factor 2, then factor 4: the second call uploads a new tap table into the buffer the first one reads."""
    inputs, outputs, step_a = _bscan_bin_io(2, "_a", 31)
    i2, o2, step_b = _bscan_bin_io(4, "_b", 32)
    inputs.update(i2), outputs.update(o2)
    return _side("bscan_bin_device, two factors", inputs, outputs, [step_a, step_b])


_add(SETTERS, "set_colormap", _colormap_case)
_add(SETTERS, "bscan_bin_device: two bin factors", _bscan_bin_factors_case)
_add(SETTERS, "set_peakhold_roi", _side_set_peakhold_roi)
_add(SETTERS, "manualavg_begin", _side_manualavg_begin)


@pytest.mark.parametrize("name", list(SETTERS))
def test_a_state_change_does_not_reach_back(name):
    case = _named("b", name, SETTERS)
    want = run_quiet(case)
    if case.setter is not None:
        first = case.main or "mag_a"          # call A's result: an output, or a hold read back when everything has run
        d = distance(want[first], run_quiet(case, "new")[first])
        DISTANCES.append((name, d))
        print("%s: quiet distance between A under the old state and A under the new: %.3g" % (name, d))
        assert case.distance is not None, name
        if case.distance == 0:
            assert d == 0, "%s: the two states are meant to give call A the same bits and are %.3g apart" % (name, d)
        else:
            assert d >= case.distance, "%s: the two states are %.3g apart in call A: a reach-back would not show" % (name, d)
    same(run_busy(case), want, name)


# ---- c. workspace growth does not reach back -------------------------------------------------------------------------------------------------
def _pair(g, io):
    """A growth pair of a side stage: io(size, suffix) for the small and the large call."""
    def build():
        inputs, outputs, step_a = io(list(g.small.values())[0], "_a")
        i2, o2, step_b = io(list(g.large.values())[0], "_b")
        inputs.update(i2), outputs.update(o2)
        case = _side("growth of %s" % g.workspace, inputs, outputs, [step_a, step_b])
        case.key = _growth_key(case.key, g)
        return case
    return build


def _complex_growth():
    g = sc.GROWTH[sc.GROWTH_IDS.index("ws_cx")]
    ch = Chain(GEN)
    na, nb = g.small["nframes"], g.large["nframes"]
    outs = {"cx_a": ((na, ch.D, ch.H), np.complex64), "cx_b": ((nb, ch.D, ch.H), np.complex64)}
    steps = [lambda r, p: r.process_complex_device(p["xa"], U16, na, 0, p["cx_a"], DXH),
             lambda r, p: r.process_complex_device(p["xb"], U16, nb, 0, p["cx_b"], DXH)]
    return Case("growth of ws_cx", _growth_key(ch.key, g), ch.make, ch.reset, {"xa": ch.frames(na), "xb": ch.frames(nb)[::-1]}, outs, steps)


for _g in sc.GROWTH:
    if _g.site in _front_chains():
        _add(GROWTH, _g.workspace, _chain_growth(_g.site, DXH if _g.workspace == "ws_tr" else HXD))
_G = {g.workspace: g for g in sc.GROWTH}
_add(GROWTH, "ws_cx", _complex_growth)
_add(GROWTH, "ws_dop_bulk", _pair(_G["ws_dop_bulk"], lambda n, s: _doppler_io(n, True, s)))
_add(GROWTH, "d_sf_part", _pair(_G["d_sf_part"], lambda n, s: _saveframes_io(n, 0, s)))
_add(GROWTH, "ws_lp_bins", _pair(_G["ws_lp_bins"], lambda rows, s: _lowpass_io(rows, sc.LOWPASS_LONG_W, s)))
_add(GROWTH, "ws_cal_mm", _pair(_G["ws_cal_mm"], _normalize_io))
_add(GROWTH, "d_disp_part", _pair(_G["d_disp_part"], lambda n, s: _display_io(n, s, 43 + n)))
_add(GROWTH, "ws_cap_mm", _pair(_G["ws_cap_mm"], lambda n, s: _side_frame_minmax(n, sfx=s)))
_add(GROWTH, "ws_col_sum", _pair(_G["ws_col_sum"], lambda n, s: _colour_io(n, 3, s)))


@pytest.mark.parametrize("name", list(GROWTH))
def test_a_workspace_that_grows_does_not_reach_back(name):
    g = _G[name]
    assert g.need(g.large) > g.need(g.small) > 0
    case = _named("c", name, GROWTH)
    want = run_quiet(case)
    same(run_busy(case), want, "call A (%s) and the larger call B (%s) of %s" % (g.small, g.large, name))


# ---- d. switching streams ----------------------------------------------------------------------------------------------------------------
def _two_streams():
    import torch
    return torch.cuda.Stream(), torch.cuda.Stream()


def test_manual_averaging_across_a_stream_switch():
    """manualavg_begin(3, count, KEEP_ALL) -- the mode in which the third image emits; two images on stalled S1, set_stream(S2), the
    third image: the emitted mean and dB are tests/manualavg_model.py's for the three images, bit for bit.  Without the order
    fdoct_set_stream gives, the third add runs at once on S2 and emits a mean that lacks the first two."""
    import torch
    rec = POOL.get(SIDE_KEY + " / busy", _side_make)
    imgs = _mavg_images(3, 63)
    model = manualavg_model.ManualAvg(3, COUNT, manualavg_model.KEEP_ALL)
    assert model.add(imgs[:2])[0].shape[0] == 0
    want_mean, want_db = model.add(imgs[2:])
    bufs = _Bufs({"two": imgs[:2], "one": imgs[2:]}, {"mean": ((1, SH, SD), np.float32), "db": ((1, SH, SD), np.float32)})
    S1, S2 = _two_streams()
    try:
        rec.set_stream(None)
        rec.manualavg_begin(3, COUNT, capi.MANUALAVG_KEEP_ALL)
        bufs.fill()
        _sync()
        assert rec.manualavg_add_device(bufs.ptr["two"], 2, None, None, 0) == 0        # warm-up of the kernel
        assert rec.manualavg_add_device(bufs.ptr["one"], 1, bufs.ptr["mean"], bufs.ptr["db"], 1) == 1
        _sync()
        rec.manualavg_begin(3, COUNT, capi.MANUALAVG_KEEP_ALL)
        bufs.poison()
        _sync()
        rec.set_stream(S1.cuda_stream)
        ev = ss.stall(S1)
        with torch.cuda.stream(S1):
            bufs.fill()
        assert rec.manualavg_add_device(bufs.ptr["two"], 2, None, None, 0) == 0
        ss.still_running(ev, "manual averaging, two images on S1")
        rec.set_stream(S2.cuda_stream)
        assert rec.manualavg_add_device(bufs.ptr["one"], 1, bufs.ptr["mean"], bufs.ptr["db"], 1) == 1
        ss.still_running(ev, "manual averaging, the emitting call on S2")
        S1.synchronize()
        S2.synchronize()
        got = bufs.read()
    finally:
        S1.synchronize()
        S2.synchronize()
        _sync()
        rec.set_stream(None)
    same(got, {"mean": want_mean, "db": want_db}, "the mean of three images across a stream switch (against the model)")


def test_peak_holds_across_a_stream_switch():
    """peakhold_device on stalled S1, set_stream(S2), peakhold_device of a second batch into the same slot: the holds are
    roi_model.PeakHold's of both batches.  (The fold is a maximum, so a second fold that ran first would give the same holds; what
    shows a wrong order is the clear in front of the first fold, enqueued on S1 behind the stall: run late, it wipes both.)"""
    import torch
    rec = POOL.get(SIDE_KEY + " / busy", _side_make)
    a, b = _db_images(2, SD, HXD, 8), _db_images(2, SD, HXD, 9) + 5.0
    model = roi_model.PeakHold()
    model.set_roi(*ROI_1)
    model.fold(1, roi_model.picture(a, HXD))
    model.fold(1, roi_model.picture(b, HXD))
    bufs = _Bufs({"a": a, "b": b}, {})
    S1, S2 = _two_streams()
    try:
        rec.set_stream(None)
        _roi_start(rec)
        bufs.fill()
        _sync()
        rec.peakhold_device(1, bufs.ptr["a"], 2, SD, SH, HXD)       # warm-up
        _sync()
        bufs.poison()
        _sync()
        rec.set_stream(S1.cuda_stream)
        ev = ss.stall(S1)
        with torch.cuda.stream(S1):
            bufs.fill()
        rec.clear_peakhold(1)
        rec.peakhold_device(1, bufs.ptr["a"], 2, SD, SH, HXD)
        ss.still_running(ev, "peak holds, the first fold on S1")
        rec.set_stream(S2.cuda_stream)
        rec.peakhold_device(1, bufs.ptr["b"], 2, SD, SH, HXD)
        ss.still_running(ev, "peak holds, the second fold on S2")
        cols, amax, count = rec.peakhold_values(1)                  # (reads on S2: waits for both)
    finally:
        S1.synchronize()
        S2.synchronize()
        _sync()
        rec.set_stream(None)
    np.testing.assert_array_equal(cols, model.cols[0].astype(np.float32))
    assert amax == np.float32(model.scalar[0]) and count == 4, (amax, model.scalar[0], count)


# ---- e. the rest ---------------------------------------------------------------------------------------------------------------------------
def test_130_launches_through_the_64_ticket_words():
    """130 process_device calls of the workgroup-per-row kernel (H = 11) behind one stall, into 130 output buffers: every output
    equals the quiet result -- two rounds of the 64 row counters, re-zeroed on the stream in front of each launch."""
    import torch
    ch = Chain(GEN)
    case = ch.case("process_device, 130 launches")
    want = run_quiet(case)
    rec = POOL.get(case.key + " / busy", case.make)
    n_calls = 130
    shp = ch.out_shape(1, HXD)
    bufs = _Bufs(case.inputs, {})
    mags = torch.empty((n_calls,) + shp, dtype=torch.float32, device="cuda")
    dbs = torch.empty((n_calls,) + shp, dtype=torch.float32, device="cuda")
    S = torch.cuda.Stream()
    try:
        _warm(case, rec, _Bufs(case.inputs, case.outputs))
        assert rec.last_kernel() == capi.KERNEL_GENERIC
        bufs.poison()
        mags.fill_(float("nan"))
        dbs.fill_(float("nan"))
        _sync()
        rec.set_stream(S.cuda_stream)
        ev = ss.stall(S)
        with torch.cuda.stream(S):
            bufs.fill()
        t0 = time.perf_counter()
        for k in range(n_calls):
            rec.process_device(bufs.ptr["x"], U16, 1, 0, mags[k].data_ptr(), dbs[k].data_ptr(), HXD)
        ms = (time.perf_counter() - t0) * 1e3
        ss.still_running(ev, "130 launches")
        S.synchronize()
        got_m, got_d = mags.cpu().numpy(), dbs.cpu().numpy()
    finally:
        S.synchronize()
        _sync()
        rec.set_stream(None)
    print("130 calls enqueued in %.2f ms behind a stall of %g ms" % (ms, ss.STALL_MS))
    bad = [k for k in range(n_calls) if got_m[k].tobytes() != want["mag"].tobytes() or got_d[k].tobytes() != want["db"].tobytes()]
    assert not bad, "launches %s differ from the quiet result" % bad[:10]


def test_close_with_a_call_in_flight():
    """close() while the handle's call waits behind the stall on the caller's stream: the caller's output holds the quiet result."""
    import torch
    ch = Chain(FAST)
    case = ch.case("process_device, then close")
    want = run_quiet(case)
    rec = ch.make()
    bufs = _Bufs(case.inputs, case.outputs)
    S = torch.cuda.Stream()
    try:
        _warm(case, rec, bufs)
        bufs.poison()
        _sync()
        rec.set_stream(S.cuda_stream)
        ev = ss.stall(S)
        with torch.cuda.stream(S):
            bufs.fill()
        case.steps[0](rec, bufs.ptr)
        ss.still_running(ev, "close with a call in flight")
        rec.close()
        S.synchronize()
        got = bufs.read()
    finally:
        S.synchronize()
        _sync()
        rec.close()
    same(got, want, "the output of a call in flight when its handle was closed")


def test_host_memory_calls_on_a_handle_whose_stream_is_stalled():
    """process() and saveframes() with host memory on both sides, on a handle whose caller's stream is busy: both return drained,
    with the quiet results."""
    import torch
    ch = Chain(FAST)
    frames = ch.frames(2)
    pics = _linear_images(2, 85)
    quiet = POOL.get(ch.key + " / quiet", ch.make)
    ch.reset(quiet)
    want = dict(zip(("mag", "db"), quiet.process(frames)))
    want.update(zip(("gray", "b", "sdb"), quiet.saveframes(pics, averages=2)))
    rec = POOL.get(ch.key + " / busy", ch.make)
    S = torch.cuda.Stream()
    try:
        ch.reset(rec)
        rec.process(frames)
        rec.saveframes(pics, averages=2)
        _sync()
        rec.set_stream(S.cuda_stream)
        ev = ss.stall(S)
        got = dict(zip(("mag", "db"), rec.process(frames)))
        first_returned_drained = ev.query()
        ev = ss.stall(S)
        got.update(zip(("gray", "b", "sdb"), rec.saveframes(pics, averages=2)))
        assert first_returned_drained and ev.query(), "a host-memory call returned with the handle's stream still busy"
    finally:
        S.synchronize()
        _sync()
        rec.set_stream(None)
    same(got, want, "host-memory process() and saveframes() behind a stall")


def test_enqueue_times_and_stall_length():
    """What the run states: the calibration, STALL_MS, the enqueue time it is derived from, the slowest case.  STALL_MS must be at
    least 100 x the slowest warm call A (measured three times on a drained device, the smallest taken; calls that keep state are
    measured once and only printed), within 10 .. 100 ms."""
    for name in RESIDENCY:            # (cached when the tests above have run)
        run_quiet(_named("a", name, RESIDENCY))
    cal = ss.calibration()
    print("stall: %s, %.0f per ms, a 10 ms stall measured %.2f ms; STALL_MS = %g" % (cal["mode"], cal["per_ms"], cal["check_ms"], ss.STALL_MS))
    for name, ms in sorted(ENQUEUE_MS.items(), key=lambda kv: -kv[1])[:8]:
        print("  call A enqueue %.3f ms (smallest of three)  %s" % (ms, name))
    for name, ms in sorted(ENQUEUE_ONCE_MS.items(), key=lambda kv: -kv[1])[:4]:
        print("  call A enqueue %.3f ms (once)  %s" % (ms, name))
    for name, ms in sorted(CASE_MS.items(), key=lambda kv: -kv[1])[:5]:
        print("  stalled case %.0f ms  %s" % (ms, name))
    for name, d in DISTANCES:
        print("  distance %.3g  %s" % (d, name))
    slowest = max(ENQUEUE_MS.values())
    need = min(100.0, max(10.0, 100.0 * slowest))
    assert ss.STALL_MS >= need, "STALL_MS = %g, the slowest call A takes %.3f ms to enqueue: at least %g ms" % (ss.STALL_MS, slowest, need)
