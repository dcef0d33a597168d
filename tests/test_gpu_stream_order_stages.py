"""The stream-order contract ("Stream order") of the five add-on stages -- the dispersion search, vibrometry, angiography,
coherent averaging and split-spectrum decorrelation -- on a busy stream.  Their entry points are module-level functions over a
Reconstructor (tests/stream_cases.py: ADDON_ENTRIES), which the catalogue of tests/test_gpu_stream_order.py does not see; this file
runs them through that file's machinery (Case, run_quiet, run_busy, same, the handle pool, the stall of tests/stream_stall.py).  Every
comparison is bit for bit against the quiet run of the same steps on a second handle; every stalled case asserts that the stall is
still running when its call A has returned, or, where call A hands a result back in host memory, that the stream is drained.

a. residency       one case per entry: inputs filled on the stalled stream, outputs NaN poison.  The process_* forms of vibrometry,
                   angiography and coherent averaging run on the chain handle of process_doppler_device; fdoct_process_ssada and
                   fdoct_process_dispersion_search refuse a handle whose numdisplaypoints is not numfftpoints, so those two run on a
                   64 x 4 handle with N = D = 128 and a background.  Two controls (ssada_device, vibro_device) leave the handle on
                   its own stream and must NOT equal the quiet run; a control counts only if the handle's stream has finished while
                   the stall still runs (run_control: two streams may share a hardware queue).
b. tables          each stage writes device tables into handle-owned memory per call, from the call's parameters.  Call A (p1) and
                   call B (p2) of stream_cases.TABLE_PAIRS -- same sizes, so nothing is reserved and nothing drains -- into separate
                   outputs behind one stall: each equals its quiet run.  The quiet distance of A's main output between p1 and p2 is
                   printed and held to FAR.
c. growth          one case per stream_cases.ADDON_GROWTH entry, on a handle pair of its own.
d. stream switch   the pairs of b with call A on stalled S1, set_stream(S2), call B on S2: the table B overwrites is the one A reads.
e. host memory     per stage a call with device input and its main output in host memory returns drained with the quiet result.
                   fdoct_ssada has one out_space for all four outputs, so "out_bands alone" is out_bands with the float outputs
                   absent: the path on which nothing but the flag fdoct_ssada.cpp sets by hand drains the call -- in one pass, and
                   in three passes that reuse the workspace between the copies down.
f. the models      once per stage the quiet result of its residency case is held to the stage's model by the stage's own
                   adjudication (ssada_model.check_bands, dispersion_model.check, vibro_model.check, angio_model.check,
                   cxavg_model.check): two runs that agree on something wrong do not pass.

No case is built so that a violation would fault: every buffer a misordered kernel could touch is the test's or the handle's."""
import ctypes as C
import time

import numpy as np
import pytest

import angio_model as am
import cxavg_model as cm
import dispersion_model as dm
import ssada_model as sm
import stream_cases as sc
import stream_stall as ss
import test_gpu_stream_order as so
import vibro_model as vm
from fdoct_amd import Config, Reconstructor, angiography, capi, coherent, dispersion, ssada, synth, vibrometry

pytestmark = pytest.mark.gpu

HOST, DEV, U16 = capi.MEM_HOST, capi.MEM_DEVICE, capi.DTYPE_U16
FAR = sc.FAR
PREFIX = "stages "        # of this file's case names: the quiet runs and the enqueue times are cached by name, next to the other file's
DISTANCES = []            # (stage, quiet distance of A's main output between p1 and p2)
OUTPUTS = {"ssada": ("decorr", "band_decorr", "power", "bands"), "dispersion": ("sums", "row_sums", "best", "cos_sin"),
           "vibro": ("amp", "rms", "drift", "power"), "angio": ("var", "decorr", "cdecorr", "power"), "cxavg": ("mean", "mag", "incoh", "coh")}


@pytest.fixture(scope="module", autouse=True)
def _handles():
    import torch
    yield
    torch.cuda.synchronize()
    so.POOL.close()


# ---- a stage's call as a value -------------------------------------------------------------------------------------------------------------
class Call:
    """One call of a stage on complex A-scans of `shape` with the model's keywords `p` (tests/stream_cases.py): the outputs' shapes,
    and the call in its three forms -- the binding's *_device function, its process_*_device function on camera frames, and the C
    entry point with the outputs in host memory.  Every form takes (rec, input pointer, [four output pointers or None])."""

    def __init__(self, stage, shape, p):
        self.stage, self.shape, self.p, self.names = stage, dict(shape), dict(p), OUTPUTS[stage]
        f32, c64 = np.float32, np.complex64
        if stage == "ssada":
            G, R, H, n, M = shape["groups"], shape["repeats"], shape["ascans"], shape["n"], p["bands"]
            dc = sm.resolve(n, M, 1.0, (0, 0), p.get("depth", (0, 0)))[4]
            par = ssada.params(n=n, **p)
            self.in_shape = (G * R, H, n)
            self.outs = {"decorr": ((G, H, dc), f32), "band_decorr": ((G, M, H, dc), f32), "power": ((G, H, dc), f32), "bands": ((G, M, R, H, dc), c64)}
            self.dev = lambda r, x, o: ssada.ssada_device(r, x, G * R, H, n, par, *o)
            self.proc = lambda r, x, o: ssada.process_ssada_device(r, x, U16, G * R, 0, par, *o)
            self.host = lambda r, x, o: r._check(r.lib.fdoct_ssada(r.h, x, DEV, G * R, H, n, C.byref(par), o[0], o[1], o[2], o[3], HOST))
        elif stage == "dispersion":
            rows, n = shape["rows"], shape["n"]
            a2, a3, depth = sc.disp_axes(p)
            K, grid = a2[2] * a3[2], dispersion.grid(a2, a3, depth)
            self.in_shape = (rows, n)
            self.outs = {"sums": ((K, 2), np.float64), "row_sums": ((rows, K, 2), np.float64), "best": ((1,), dispersion.BEST_DTYPE), "cos_sin": ((n, 2), f32)}
            self.dev = lambda r, x, o: dispersion.search_device(r, x, rows, n, a2, a3, *o, depth=depth)
            self.proc = lambda r, x, o: dispersion.process_search_device(r, x, U16, shape["nframes"], 0, a2, a3, *o, depth=depth)
            self.host = lambda r, x, o: r._check(r.lib.fdoct_dispersion_search(r.h, x, DEV, rows, n, C.byref(grid), o[0], o[1], o[2], o[3], HOST))
        else:
            T, H, D = shape["nframes"], shape["ascans"], shape["depths"]
            self.in_shape = (T, H, D)
            if stage == "vibro":
                par, mod, fn = vibrometry.params(**p), vibrometry, "vibro"
                self.outs = {"amp": ((len(p.get("freq", ())), H, D), c64), "rms": ((H, D), f32), "drift": ((H, D), f32), "power": ((H, D), f32)}
            elif stage == "angio":
                par, mod, fn = angiography.params(**p), angiography, "angio"
                self.outs = {w: ((T // p["repeats"], H, D), f32) for w in self.names}
            else:
                par, mod, fn = coherent.params(**p), coherent, "cxavg"
                G = (T - p["repeats"]) // (p.get("stride") or p["repeats"]) + 1
                self.outs = {w: ((G, H, D), c64 if w == "mean" else f32) for w in self.names}
            self.dev = lambda r, x, o: getattr(mod, fn + "_device")(r, x, T, H, D, par, *o)
            self.proc = lambda r, x, o: getattr(mod, "process_%s_device" % fn)(r, x, U16, T, 0, par, *o)
            self.host = lambda r, x, o: r._check(getattr(r.lib, "fdoct_" + fn)(r.h, x, DEV, T, H, D, C.byref(par), o[0], o[1], o[2], o[3], HOST))

    def io(self, want=None, sfx="", seed=1, form="dev", frames=None):
        """(inputs, outputs, step) of the call into device memory: the buffers are named with `sfx`."""
        want = self.names if want is None else want
        X = frames if frames is not None else sc.addon_field(self.stage, self.shape, seed)
        assert frames is not None or X.shape == self.in_shape, (X.shape, self.in_shape)
        call = self.dev if form == "dev" else self.proc
        names = self.names
        step = lambda r, q: call(r, q["x" + sfx], [q[w + sfx] if w in want else None for w in names])   # noqa: E731
        return {"x" + sfx: X}, {w + sfx: self.outs[w] for w in want}, step

    def host_step(self, want, sfx=""):
        """The step that hands `want` (one output) back in host memory, as the floats (or bytes) the library wrote."""
        shape, dt = self.outs[want]
        names, host = self.names, self.host

        def step(r, q):
            out = np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, 0xFF, np.uint8)
            host(r, q["x" + sfx], [out.ctypes.data if w == want else None for w in names])
            return out
        return step


def _stage_case(name, inputs, outputs, steps, **kw):
    """A case on the side stages' handle pair (the stages alone read nothing of a handle's geometry)."""
    return so._side(name, inputs, outputs, steps, **kw)


# ---- f. the quiet result against the stage's model ----------------------------------------------------------------------------------------
def _best_dict(best):
    b = best[0]
    return {k: (int(b[k]) if k in ("index", "i2", "i3") else float(b[k])) for k in ("index", "i2", "i3", "a2", "a3", "metric")}


def _model_check(call, X, what):
    stage, p = call.stage, call.p

    def check(rec, out):
        if stage == "ssada":
            sm.check_bands(out["bands"], sm.model(X, truth=True, **p), sm.model(X, **p), call.shape["n"], what)
        elif stage == "dispersion":
            a2, a3, depth = sc.disp_axes(p)
            dm.check(dict(out, best=_best_dict(out["best"])), X, a2, a3, depth, what)
        elif stage == "vibro":
            vm.check(out, X, what, **p)
        elif stage == "angio":
            am.check(out, X, what, **p)
        else:
            cm.check(out, X, what, **p)
        MODEL_CHECKED.append(stage)
    return check


MODEL_CHECKED = []

# ---- a. residency ---------------------------------------------------------------------------------------------------------------------------
RESIDENCY, TABLES, ALT, GROWTH, HOST_CASES = {}, {}, {}, {}, {}
ENTRY_OF = {"ssada": "ssada.ssada_device", "dispersion": "dispersion.search_device", "vibro": "vibrometry.vibro_device",
            "angio": "angiography.angio_device", "cxavg": "coherent.cxavg_device"}
PROCESS_OF = {"ssada": "ssada.process_ssada_device", "dispersion": "dispersion.process_search_device", "vibro": "vibrometry.process_vibro_device",
              "angio": "angiography.process_angio_device", "cxavg": "coherent.process_cxavg_device"}
PAIR = {t.stage: t for t in sc.TABLE_PAIRS}


def _device_case(stage):
    def build():
        t = PAIR[stage]
        call = Call(stage, t.shape, t.p1)
        inputs, outputs, step = call.io(seed=t.seed)
        what = "%s, quiet run behind no stall" % ENTRY_OF[stage]
        return _stage_case(ENTRY_OF[stage], inputs, outputs, [step], check=_model_check(call, inputs["x"], what))
    return build


for _stage in sc.ADDON_STAGES:
    so._add(RESIDENCY, ENTRY_OF[_stage], _device_case(_stage))

# the chain forms: vibrometry, angiography and coherent averaging behind the chain of process_doppler_device's handle ...
CHAIN_P = {"vibro": dict(freq=(0.11, 0.25), ref=(20, 4), chunk_steps=2), "angio": dict(repeats=2, win=(3, 5), bulk=(10, 100)),
           "cxavg": dict(repeats=2, ref=1, align=2, align_range=(10, 100))}
CHAIN_FRAMES = 4


def _chain_case(stage):
    def build():
        ch = so.Chain(so.GEN)
        call = Call(stage, dict(nframes=CHAIN_FRAMES, repeats=2, ascans=ch.H, depths=ch.D), CHAIN_P[stage])
        inputs, outputs, step = call.io(form="proc", frames=ch.frames(CHAIN_FRAMES))
        return so.Case(PROCESS_OF[stage], ch.key, ch.make, ch.reset, inputs, outputs, [step])
    return build


# ... and the two that need the full transform length, on a small handle of their own
FW, FH, FN = 64, 4, 128
FULL_KEY = "full length, 64 x 4, N = D = 128"
FULL = {"ssada": (dict(groups=2, repeats=2, ascans=FH, n=FN), dict(repeats=2, bands=3, support=(4, 100), depth=(3, 41), win=(3, 5))),
        "dispersion": (dict(nframes=2, rows=2 * FH, n=FN), dict(a2=(-8.0, 8.0), a3=(0.0, 2.0), grid=(3, 1), depth=(2, 0)))}


def _full_make():
    rec = Reconstructor(Config(width=FW, height=FH, numfftpoints=FN, numdisplaypoints=FN))
    rec.set_background(synth.make_background(FW))
    return rec


def _full_case(stage):
    def build():
        shape, p = FULL[stage]
        call = Call(stage, shape, p)
        nframes = shape["groups"] * shape["repeats"] if stage == "ssada" else shape["nframes"]
        frames = synth.make_frames(4, nframes, FW, FH, dtype=np.uint16)
        inputs, outputs, step = call.io(form="proc", frames=frames)
        return so.Case(PROCESS_OF[stage], FULL_KEY, _full_make, lambda rec: rec.set_stream(None), inputs, outputs, [step])
    return build


for _stage in sc.ADDON_STAGES:
    so._add(RESIDENCY, PROCESS_OF[_stage], (_full_case if _stage in FULL else _chain_case)(_stage))


# ---- b / d. two calls that share a table ----------------------------------------------------------------------------------------------------
TABLE_WANT = {"ssada": ("decorr", "band_decorr", "power")}     # without a device out_bands the band pairs lie in ws_ssa


def _table_case(t):
    def build():
        want = TABLE_WANT.get(t.stage)
        ia, oa, step_a = Call(t.stage, t.shape, t.p1).io(want, "_a", t.seed)
        ib, ob, step_b = Call(t.stage, t.shape, t.p2).io(want, "_b", t.seed + 50)
        ia.update(ib), oa.update(ob)
        return _stage_case("%s, p1 then p2" % t.stage, ia, oa, [step_a, step_b], main=t.main + "_a")
    return build


def _alt_case(t):
    """Call A's input under p2, alone: what a reach-back would make of call A."""
    def build():
        inputs, outputs, step = Call(t.stage, t.shape, t.p2).io(TABLE_WANT.get(t.stage), "_a", t.seed)
        return _stage_case("%s, p2 on call A's input" % t.stage, inputs, outputs, [step])
    return build


for _t in sc.TABLE_PAIRS:
    so._add(TABLES, _t.stage, _table_case(_t))
    so._add(ALT, _t.stage, _alt_case(_t))


# ---- c. growth ----------------------------------------------------------------------------------------------------------------------------------
def _growth_case(g):
    def build():
        sa, shape_a, pa, want = sc.addon_call(g, g.small)
        sb, shape_b, pb, _ = sc.addon_call(g, g.large)
        ia, oa, step_a = Call(sa, shape_a, pa).io(want, "_a", 300 + sc.ADDON_GROWTH_IDS.index(g.workspace))
        ib, ob, step_b = Call(sb, shape_b, pb).io(want, "_b", 350 + sc.ADDON_GROWTH_IDS.index(g.workspace))
        ia.update(ib), oa.update(ob)
        case = _stage_case("growth of %s" % g.workspace, ia, oa, [step_a, step_b])
        case.key = so._growth_key(case.key, g)
        return case
    return build


for _g in sc.ADDON_GROWTH:
    so._add(GROWTH, _g.workspace, _growth_case(_g))
_G = {g.workspace: g for g in sc.ADDON_GROWTH}


# ---- e. host memory -------------------------------------------------------------------------------------------------------------------------------
def _host_case(name, stage, shape, p, want, seed):
    def build():
        call = Call(stage, shape, p)
        inputs, _, _ = call.io((), "", seed)
        return _stage_case(name, inputs, {}, [call.host_step(want)], drains=True)
    return build


for _t in sc.TABLE_PAIRS:
    so._add(HOST_CASES, "%s: %s in host memory" % (_t.stage, _t.main), _host_case("%s, %s in host memory" % (_t.stage, _t.main), _t.stage, _t.shape, _t.p1, _t.main, _t.seed + 7))
SSA3 = dict(groups=3, repeats=2, ascans=3, n=60)
SSA3_P = dict(repeats=2, bands=3, win=(1, 1))
SSA3_SHARE = sc.ssada_bytes(dict(SSA3, groups=1), SSA3_P)["ws_ssa"]
so._add(HOST_CASES, "ssada: out_bands alone in host memory", _host_case("ssada, out_bands alone in host memory", "ssada", SSA3, SSA3_P, "bands", 221))
so._add(HOST_CASES, "ssada: out_bands alone in host memory, three passes",
        _host_case("ssada, out_bands alone in host memory, three passes", "ssada", SSA3, dict(SSA3_P, max_workspace_bytes=SSA3_SHARE), "bands", 221))


def _named(group, name, reg):
    return so._named(PREFIX + group, name, reg)


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------------
def test_the_catalogue_has_a_case_for_every_addon_name():
    assert sorted(RESIDENCY) == sorted(sc.ADDON_ENTRIES), (sorted(set(sc.ADDON_ENTRIES) - set(RESIDENCY)), sorted(set(RESIDENCY) - set(sc.ADDON_ENTRIES)))
    assert sorted(TABLES) == sorted(sc.TABLE_PAIR_IDS) == sorted(ALT) == sorted(sc.ADDON_STAGES)
    assert sorted(GROWTH) == sorted(sc.ADDON_GROWTH_IDS)
    for stage in sc.ADDON_STAGES:
        assert [n for n in HOST_CASES if n.startswith(stage + ":")], stage
    assert len([n for n in HOST_CASES if n.startswith("ssada:")]) == 3
    assert all(build().drains for build in HOST_CASES.values())


@pytest.mark.parametrize("name", list(RESIDENCY))
def test_every_addon_entry_does_its_device_work_on_the_handles_stream(name):
    case = _named("a", name, RESIDENCY)
    want = so.run_quiet(case)
    so.same(so.run_busy(case), want, name)


CONTROL_TRIES = 8


def run_control(case):
    """The residency control: the producer on a stalled stream S, the handle left on its own stream.  The control shows something
    only if the handle's stream really runs while S is stalled, and that is the runtime's to decide: a process has a few hardware
    queues (four by default) and gives each stream one of them, so two streams may share a queue, and work on the handle's stream
    then waits behind the stall like work on S itself -- the call sees its inputs after all, by timing.  So the run says which
    happened: when the call has returned, the handle's stream is waited for (fdoct_synchronize), and the run counts only if the
    stall is still running after that -- the call's work is then over before the inputs were filled.  Otherwise the same steps are
    taken with another stream as S, up to CONTROL_TRIES times.  Returns (outputs, the number of streams tried)."""
    import torch
    rec = so.POOL.get(case.key + " / busy", case.make)
    for attempt in range(1, CONTROL_TRIES + 1):
        S = torch.cuda.Stream()
        bufs = so._Bufs(case.inputs, case.outputs)
        try:
            so._warm(case, rec, bufs)          # (leaves the handle on its own stream)
            bufs.poison()
            so._sync()
            ev = ss.stall(S)
            with torch.cuda.stream(S):
                bufs.fill()
            rets = [case.steps[0](rec, bufs.ptr)]
            ss.still_running(ev, case.name + ", control")
            rec.synchronize()
            ran_beside_the_stall = not ev.query()
            S.synchronize()
            out = so._collect(case, rec, bufs, rets)
        finally:
            S.synchronize()
            so._sync()
        if ran_beside_the_stall:
            return out, attempt
    raise AssertionError("%s: on none of %d streams did the handle's own stream run beside the stall: the control shows nothing" % (case.name, CONTROL_TRIES))


@pytest.mark.parametrize("name", ["ssada.ssada_device", "vibrometry.vibro_device"])
def test_residency_control_a_handle_left_on_its_own_stream_consumes_poison(name):
    """The producer on the stalled stream, the handle on its own, the handle's work over while the stall still runs (run_control):
    the result must NOT equal the quiet run.  This is what the comparison of the test above looks like when it fails."""
    case = _named("a", name, RESIDENCY)
    want = so.run_quiet(case)
    got, tried = run_control(case)
    bad = so.differences(got, want)
    print("%s, handle on its own stream (stream %d of at most %d ran beside the stall): %s" % (name, tried, CONTROL_TRIES, "; ".join(bad)))
    assert bad, name + ": a call that cannot have seen its inputs equals the quiet run"


@pytest.mark.parametrize("stage", sc.ADDON_STAGES)
def test_the_quiet_residency_result_was_held_to_the_stages_model(stage):
    so.run_quiet(_named("a", ENTRY_OF[stage], RESIDENCY))      # (cached when the residency test has run; its check ran with it)
    assert stage in MODEL_CHECKED, stage


def _quiet_pair(stage):
    case = _named("b", stage, TABLES)
    want = so.run_quiet(case)
    return case, want


@pytest.mark.parametrize("stage", sc.TABLE_PAIR_IDS)
def test_a_table_the_next_call_rewrites_does_not_reach_back(stage):
    case, want = _quiet_pair(stage)
    alt = so.run_quiet(_named("b, p2 alone", stage, ALT))
    d = sc.distance(want[case.main], alt[case.main])
    DISTANCES.append((stage, d))
    print("%s: quiet distance of %s between call A under p1 and under p2: %.3g" % (stage, case.main, d))
    assert d >= FAR, "%s: the two parameter sets are %.3g apart in call A: a reach-back would not show" % (stage, d)
    so.same(so.run_busy(case), want, "%s: call A (p1) and call B (p2)" % stage)


@pytest.mark.parametrize("name", list(GROWTH))
def test_an_addon_workspace_that_grows_does_not_reach_back(name):
    g = _G[name]
    assert g.need(g, g.large) > g.need(g, g.small) > 0
    case = _named("c", name, GROWTH)
    want = so.run_quiet(case)
    so.same(so.run_busy(case), want, "call A (%s) and the larger call B (%s) of %s" % (g.small, g.large, name))


def run_switch(case):
    """Call A on stalled S1, set_stream(S2), call B on S2; every input is filled on S1 behind the stall."""
    import torch
    rec = so.POOL.get(case.key + " / busy", case.make)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = so._Bufs(case.inputs, case.outputs)
    t_case = time.perf_counter()
    try:
        so._warm(case, rec, bufs)
        bufs.poison()
        so._sync()
        rec.set_stream(S1.cuda_stream)
        ev = ss.stall(S1)
        with torch.cuda.stream(S1):
            bufs.fill()
        rets = [case.steps[0](rec, bufs.ptr)]
        ss.still_running(ev, case.name + ": call A on S1")
        rec.set_stream(S2.cuda_stream)
        rets.append(case.steps[1](rec, bufs.ptr))
        ss.still_running(ev, case.name + ": call B on S2")
        S1.synchronize()
        S2.synchronize()
        rec.synchronize()
        return so._collect(case, rec, bufs, rets)
    finally:
        S1.synchronize()
        S2.synchronize()
        so._sync()
        rec.set_stream(None)
        so.CASE_MS[case.name + ", stream switch"] = (time.perf_counter() - t_case) * 1e3


@pytest.mark.parametrize("stage", sc.TABLE_PAIR_IDS)
def test_a_stream_switch_between_two_calls_that_share_a_table(stage):
    case, want = _quiet_pair(stage)
    so.same(run_switch(case), want, "%s: call A (p1) on S1, set_stream, call B (p2) on S2" % stage)


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_a_host_memory_output_returns_drained(name):
    case = _named("e", name, HOST_CASES)
    want = so.run_quiet(case)
    assert not (want["returned by step 0"] == 0xFF).all(), name + ": nothing was written"
    so.same(so.run_busy(case), want, name)


def test_three_passes_and_one_give_out_bands_the_same_bits():
    """(The two SSADA cases of group e differ in the passes alone: include/fdoct_ssada.h promises the same bits.)"""
    assert ssada.plan(dict(SSA3_P, n=60), 6, 3, 60)["passes"] == 1 and ssada.plan(dict(SSA3_P, max_workspace_bytes=SSA3_SHARE, n=60), 6, 3, 60)["passes"] == 3
    one = so.run_quiet(_named("e", "ssada: out_bands alone in host memory", HOST_CASES))
    three = so.run_quiet(_named("e", "ssada: out_bands alone in host memory, three passes", HOST_CASES))
    so.same(three, one, "out_bands in three passes against one")


def test_addon_enqueue_times_and_stall_length():
    """The warm host-side enqueue time of every call A of this file (the smallest of three on a drained device), the ten entries'
    first; STALL_MS must be at least 100 x the slowest, within 10 .. 100 ms.  The calls of group e return drained by contract: their
    time is a round trip, not an enqueue, and the stall need not outlast it -- printed, and left out of the rule."""
    for name in RESIDENCY:            # (cached when the tests above have run)
        so.run_quiet(_named("a", name, RESIDENCY))
    mine = {k: v for k, v in so.ENQUEUE_MS.items() if k.startswith(PREFIX)}
    entries = {k: v for k, v in mine.items() if k.startswith(PREFIX + "a. ")}
    assert len(entries) == len(sc.ADDON_ENTRIES)
    cal = ss.calibration()
    print("stall: %s, %.0f per ms, a 10 ms stall measured %.2f ms; STALL_MS = %g" % (cal["mode"], cal["per_ms"], cal["check_ms"], ss.STALL_MS))
    for name, ms in sorted(entries.items(), key=lambda kv: -kv[1]):
        print("  call A enqueue %.3f ms (smallest of three)  %s" % (ms, name))
    for name, ms in sorted(mine.items(), key=lambda kv: -kv[1]):
        if name not in entries:
            print("  call A %s %.3f ms (smallest of three)  %s" % ("round trip" if name.startswith(PREFIX + "e. ") else "enqueue", ms, name))
    for name, ms in sorted(so.CASE_MS.items(), key=lambda kv: -kv[1]):
        if name.startswith(PREFIX):
            print("  stalled case %.0f ms  %s" % (ms, name))
    for stage, d in DISTANCES:
        print("  distance %.3g  %s" % (d, stage))
    slowest = max(v for k, v in mine.items() if not k.startswith(PREFIX + "e. "))
    need = min(100.0, max(10.0, 100.0 * slowest))
    assert ss.STALL_MS >= need, "STALL_MS = %g, the slowest call A takes %.3f ms to enqueue: at least %g ms" % (ss.STALL_MS, slowest, need)
