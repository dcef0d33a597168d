"""The long-row path (fdoct_big.hip; big_idft and run_big in fdoct_big_host.cpp) where the rest of the suite does not reach: transforms
of three grouped launches -- the middle launch is the only one with P > 1 and F > 1, where a tile of 16 sub-problems crosses a
multiple of P and the store k1 + P (a Q + e) and the twiddle index (k1 + P k) twstep are non-trivial together --, every pairing of
{even launches, odd launches, chirp} of the last two transforms of the chain (which of the two buffers each transform may
overwrite), batches cut into several chunks (FDOCT_BIG_CHUNK_MB), and the one-launch-per-pass form (FDOCT_BIG_PER_PASS).

Every case runs the whole chain, is asserted to have run on the long-row path, and is held to helpers.oracle_reference with
check_mag (which adjudicates against the chain in double) and check_db, in both layouts.  What the cases claim about their
transforms -- three launches, the pairings -- is read from tests/native/bigplan_check.expected, the table the planner itself
printed (tests/test_abi.py pins it), by a test that needs no GPU.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
from fdoct_amd import LAYOUT_TRANSPOSED, VARIANT_SIM, Config, Reconstructor, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def case(name, W, M, N, D, A=1, H=2, dtype="u16", force=False, three=(), **opts):
    """force: the library would run this geometry elsewhere, the long-row path is asked for (fdoct_set_plan(h, -3)).
    three: the transform lengths of the case that the docstrings claim to take three grouped launches.
    opts: sim, rownorm, dark, bandpass, phase."""
    return dict(name=name, W=W, M=M, N=N, D=D, A=A, H=H, dtype=dtype, force=force, three=tuple(three), opts=opts)


# ---- transforms of three grouped launches (plans: bigplan_check.expected)
THREE_LAUNCH_CASES = [
    # groups 64 x 64 x 32; the resample loader fused into group 0 (F = 2048), the crop in group 2
    case("131072 = 2^17", 2048, 1, 131072, 2048, A=2, H=3, three=[131072]),
    # radix 5 only: P = 125, then 3125, the last tile of every group short, no Ns a power of two
    case("78125 = 5^7", 640, 1, 78125, 777, A=3, H=2, dtype="u8", three=[78125]),
    # the smallest length of three groups; radices 3 and 2 in the middle group; display beyond N / 2; the minmax table
    case("65610 = 2 3^8 5", 1000, 1, 65610, 40000, A=1, H=3, dtype="f32", sim=True, three=[65610]),
    # complex rows
    case("98304 = 2^15 3 with a phase", 2048, 1, 98304, 60000, A=2, H=2, dtype="f64", phase=True, three=[98304]),
    # M W = 131072: the re-packing loader fused into a three-launch transform, with the band-pass, a dark frame, row-wise normalisation
    case("16384 x 8 -> 131072", 16384, 8, 8192, 1024, A=1, H=2, bandpass=True, dark=True, rownorm=True, three=[131072]),
    case("3000 x 32 -> 96000 = 2^8 3 5^3", 3000, 32, 3000, 1500, A=2, H=2, dtype="u8", three=[96000]),
    # chirp (Bluestein) around 131072: both inner transforms have three launches, the materialised loaders run in front
    case("57344 = 7 2^13, chirp", 1000, 1, 57344, 1000, A=1, H=3, three=[57344]),
    case("34816 = 17 2^11, chirp", 2048, 1, 34816, 2048, A=2, H=2, dtype="f32", dark=True, three=[34816]),
    # W is a chirp around 16384, M W = 35840 one around 131072
    case("4480 x 8 -> 35840, chirps", 4480, 8, 4096, 2048, A=1, H=2, three=[35840]),
]

# ---- the hand-over of the two buffers: (kind of the M W-point transform, kind of the N-point one), all nine pairs, small lengths
# that the library would run in LDS forced onto this path; with M = 1 only the N-point transform runs
HANDOVER_CASES = [
    case("odd > odd", 64, 4, 256, 100, A=2, force=True),
    case("odd > even", 64, 4, 1000, 700, A=1, force=True, dtype="u8"),
    case("odd > chirp", 64, 4, 448, 224, A=3, force=True, dark=True),
    case("even > odd", 250, 4, 243, 121, A=1, force=True, sim=True),
    case("even > even", 256, 4, 1024, 512, A=2, force=True, dtype="f64"),
    case("even > chirp", 250, 4, 1001, 500, A=1, force=True, rownorm=True, dark=True),
    case("chirp > odd", 56, 4, 250, 125, A=2, force=True, dtype="f32"),
    case("chirp > even", 56, 4, 1024, 1000, A=1, force=True, bandpass=True),
    case("chirp > chirp", 56, 4, 448, 200, A=2, force=True, phase=True),
    # More rows than the device holds workgroups of at once.  A transform that reads its source rows from the buffer it writes goes
    # unnoticed while every workgroup has loaded before any has stored -- which is what a few short rows do; here the launch runs
    # in several turns (36 rows x 128 tiles of the fused first launch, 48 rows x 224 blocks of the materialised loader, against
    # 256 CUs x 8 workgroups), the first turn's stores cover every source row (row r of N values lies over the rows r N / M W of
    # M W values), and the later turns would read them.
    case("even > odd, launches of several turns", 512, 8, 131072, 600, A=6, H=3, three=[131072]),
    case("even > chirp, launches of several turns", 512, 8, 57344, 600, A=8, H=3, dtype="u8", three=[57344]),
    case("one transform, odd", 100, 1, 243, 243, A=2, force=True),
    case("one transform, chirp", 100, 1, 448, 100, A=1, force=True, dtype="u8"),
]
WANT_PAIRS = {(a, b) for a in ("even", "odd", "chirp") for b in ("even", "odd", "chirp")}

# ---- chunked batches: five averaging groups, a budget that holds two of them (chunks 2, 2, 1) and one below a group (the clamp)
CHUNK_GROUPS, CHUNK_BUDGETS_MB = 5, {"4": "2,2,1", "1": "1,1,1,1,1"}
CHUNK_CASES = [
    case("two averages", 512, 8, 16384, 1024, A=2, H=3, force=True),
    case("sim variant", 512, 8, 32768, 1024, A=1, H=3, force=True, sim=True),
    case("f64 frames", 512, 8, 32768, 1024, A=1, H=3, force=True, dtype="f64", dark=True),
    case("device frames at a padded pitch", 512, 8, 16384, 1024, A=2, H=3, force=True),
]

# ---- the one-launch-per-pass form, in a child process: a length of three groups and a zero-pad geometry
PER_PASS_CASES = [
    case("per pass, 65610", 1000, 1, 65610, 2000, A=2, H=2, three=[65610]),
    case("per pass, 640 x 4 -> 2560", 640, 4, 2560, 320, A=2, H=3, force=True, bandpass=True),
]


def _lengths(c):
    """The transform lengths of a case, in the order run_big runs them."""
    W, M, N = c["W"], c["M"], c["N"]
    MW = W + 2 * ((W * M - W) // 2)
    return ([W, MW] if M > 1 else []) + [N]


def _plan_table():
    """bigplan_check.expected as {n: (kind, launches)}, kind "grouped" or "chirp", and {(W, M, N, H, A, G, mb): chunk sequence}."""
    plans, chunks = {}, {}
    for line in open(os.path.join(ROOT, "tests", "native", "bigplan_check.expected")):
        m = re.match(r"n=(\d+) (grouped|chirp)(?: mb=\d+)? launches=(\d+) ", line)
        if m:
            plans[int(m.group(1))] = (m.group(2), int(m.group(3)))
        m = re.match(r"chunks W=(\d+) M=(\d+) N=(\d+) H=(\d+) A=(\d+) G=(\d+) mb=(\d+): .* seq=([\d,]+)$", line)
        if m:
            chunks[tuple(int(x) for x in m.groups()[:7])] = m.group(8)
    return plans, chunks


def _kind(plans, n):
    kind, launches = plans[n]
    return "chirp" if kind == "chirp" else ("even" if launches % 2 == 0 else "odd")


def test_the_case_tables_reach_what_they_claim():
    """From the planner's own table (no GPU): every transform length of every case is in it; each length named as a three-launch
    transform has three launches, grouped or inside its chirp; the M > 1 cases reach all nine pairs of {even, odd, chirp} for the
    last two transforms, the M = 1 cases an odd-launch and a chirp N; a middle group with P not a power of two and a short
    last tile is among them; the chunked batches are cut as 2, 2, 1 and 1, 1, 1, 1, 1; every case is small (H <= 3)."""
    plans, chunks = _plan_table()
    cases = THREE_LAUNCH_CASES + HANDOVER_CASES + CHUNK_CASES + PER_PASS_CASES
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        assert c["H"] <= 3 and c["D"] <= c["N"], c["name"]
        for n in _lengths(c):
            assert n in plans, "%s: length %d is not in bigplan_check.expected" % (c["name"], n)
        for n in c["three"]:
            assert n in _lengths(c) and plans[n][1] == 3, (c["name"], n, plans[n])
    for c in THREE_LAUNCH_CASES:
        assert c["three"], c["name"]
    assert {plans[c["three"][0]][0] for c in THREE_LAUNCH_CASES} == {"grouped", "chirp"}
    pairs = {(_kind(plans, _lengths(c)[1]), _kind(plans, c["N"])) for c in THREE_LAUNCH_CASES + HANDOVER_CASES if c["M"] > 1}
    assert pairs == WANT_PAIRS, WANT_PAIRS - pairs
    for c in HANDOVER_CASES:  # the names are the claims
        if c["M"] > 1:
            assert c["name"].startswith("%s > %s" % (_kind(plans, _lengths(c)[1]), _kind(plans, c["N"]))), c["name"]
    single = {_kind(plans, c["N"]) for c in THREE_LAUNCH_CASES + HANDOVER_CASES if c["M"] == 1}
    assert {"odd", "chirp"} <= single, single
    # one-launch transforms among the odd ones, next to the three-launch ones
    assert {plans[n][1] for c in HANDOVER_CASES for n in _lengths(c) if plans[n][0] == "grouped"} >= {1, 2}
    text = open(os.path.join(ROOT, "tests", "native", "bigplan_check.expected")).read()
    assert re.search(r"^n=78125 grouped launches=3 \| P=1 Q=125 .* tail=short \| P=125 Q=25 F=25 .* tail=short \| P=3125 ", text, re.M)
    assert re.search(r"^n=65610 grouped launches=3 \| .* \| P=45 Q=54 F=27 log2ts=4 rad=3,3,3,2 tail=short \| ", text, re.M)
    for c in CHUNK_CASES:
        key = (c["W"], c["M"], c["N"], c["H"], c["A"], CHUNK_GROUPS)
        assert chunks[key + (0,)] == str(CHUNK_GROUPS), c["name"]          # the default budget: one chunk
        for mb, seq in CHUNK_BUDGETS_MB.items():
            assert chunks[key + (int(mb),)] == seq, (c["name"], mb, chunks[key + (int(mb),)])


# ---- inputs, the library's run and the oracle's of one case ----------------------------------------------------------
def _inputs(c, groups=2, seed=31):
    """cfg, the frames as the oracle takes them (u16 / u8), the same frames in the case's dtype, the background, the oracle's keywords."""
    W, H, N, D, M, A, o = c["W"], c["H"], c["N"], c["D"], c["M"], c["A"], c["opts"]
    ckw = dict(variant=VARIANT_SIM) if o.get("sim") else {}
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, averages=A,
                 rowwisenormalize=1 if o.get("rownorm") else 0, **ckw)
    u8 = c["dtype"] == "u8"
    frames = synth.make_frames(seed, groups * A, W, H, dtype=np.uint8 if u8 else np.uint16)
    yb = synth.make_background(W, dtype=np.uint8 if u8 else np.uint16).astype(np.float64) + (1.0 if u8 else 10.0)
    if o.get("sim") or o.get("rownorm"):
        yb = yb / (255.0 if u8 else 65535.0)
    kw = {}
    if o.get("phase"):
        kw["phase"] = synth.dispersion_phase(N)
    if o.get("dark"):
        kw["yd"] = 0.02 * float(frames.max()) * np.random.default_rng(3).random((H, W))
    if o.get("bandpass"):
        kw["bandpass"] = 1
    given = frames.astype({"f32": np.float32, "f64": np.float64}[c["dtype"]]) if c["dtype"] in ("f32", "f64") else frames
    return cfg, frames, given, yb, kw


def _handle(c, cfg, yb, kw):
    r = Reconstructor(cfg)
    r.set_background(yb)
    if "phase" in kw:
        r.set_dispersion_phase(kw["phase"])
    if "yd" in kw:
        r.set_dark(kw["yd"])
    if "bandpass" in kw:
        r.set_bandpass(True)
    if c["force"]:
        r.set_plan(-3)
    return r


def _process_both_layouts(r, c, given):
    """Row-major outputs of one call; the transposed layout must be their transpose bit for bit."""
    b, d = r.process(given)
    assert r.last_kernel() == capi.KERNEL_LONG_ROWS, (c["name"], r.last_kernel(), r.jit_note())
    bt, dt = r.process(given, layout=LAYOUT_TRANSPOSED)
    assert r.last_kernel() == capi.KERNEL_LONG_ROWS
    np.testing.assert_array_equal(bt, np.transpose(b, (0, 2, 1)))
    np.testing.assert_array_equal(dt, np.transpose(d, (0, 2, 1)))
    return b, d


def _hold_to_oracle(c, cfg, frames, yb, kw, b, d, what):
    mag_o, _, db_o = helpers.oracle_reference(cfg, frames, yb, **kw)
    w = helpers.check_mag(b, mag_o, what)
    helpers.check_db(d, np.transpose(db_o, (0, 2, 1)), mag_o, what)
    return w


def _run_case(c):
    cfg, frames, given, yb, kw = _inputs(c)
    r = _handle(c, cfg, yb, kw)
    b, d = _process_both_layouts(r, c, given)
    r.close()
    what = "long rows, %s: W=%d M=%d N=%d D=%d A=%d %s %s" % (c["name"], c["W"], c["M"], c["N"], c["D"], c["A"], c["dtype"], sorted(c["opts"]))
    w = _hold_to_oracle(c, cfg, frames, yb, kw, b, d, what)
    print("%s: worst error / tolerance %.3f" % (what, w))


@gpu
@pytest.mark.parametrize("c", THREE_LAUNCH_CASES, ids=[c["name"] for c in THREE_LAUNCH_CASES])
def test_transforms_of_three_grouped_launches(c):
    """A transform above 65 536 points is three launches; the middle one has P > 1 and F > 1.  Powers of two, radix 5 alone
    (P = 125, 3125: `% P` and `/ P` inside a tile, every last tile short), radices 3 and 2 in the middle group, complex rows, the
    re-packing loader of the zero-pad stage fused into the first launch, and chirp transforms around 131072 whose loaders are
    materialised -- over the sample types, averages of 1, 2 and 3, the sim variant's minmax table, row-wise normalisation, a dark
    frame, the band-pass and a display beyond numfftpoints / 2."""
    _run_case(c)


@gpu
@pytest.mark.parametrize("c", HANDOVER_CASES, ids=[c["name"] for c in HANDOVER_CASES])
def test_buffer_hand_over_between_the_last_two_transforms(c):
    """run_big gives each transform one buffer to read and one it may overwrite; which is which depends on where the previous
    transform ended (the parity of its launches, or a chirp's fixed end) and on whether the next one fuses its loader (grouped)
    or materialises it (chirp).  A wrong choice reads rows the running launch overwrites.  All nine pairs, and a single
    transform of an odd launch count and a chirp; lengths of one launch (<= 256 points) are forced onto this path.  Two pairs run
    once more on enough rows for their launches to take several turns of the device: only then does a launch that overwrites
    its own source read what it has overwritten."""
    _run_case(c)


def _group_frames_differ(frames, A, lo=None):
    G = frames.shape[0] // A
    for g in range(G):
        for k in range(g + 1, G):
            assert not np.array_equal(frames[g * A:(g + 1) * A], frames[k * A:(k + 1) * A]), (g, k)
            if lo is not None:
                assert not np.array_equal(lo[g * A:(g + 1) * A], lo[k * A:(k + 1) * A]), (g, k)


@gpu
@pytest.mark.parametrize("c", CHUNK_CASES, ids=[c["name"] for c in CHUNK_CASES])
def test_batches_cut_into_chunks_equal_the_uncut_batch(c, monkeypatch):
    """run_big cuts a batch into chunks of whole averaging groups that fit its workspace budget (2 GiB; FDOCT_BIG_CHUNK_MB, read
    at every call).  Five groups under a budget of two groups (chunks 2, 2, 1: a second turn and a ragged last one) and under a
    budget below one group (the clamp to one) must give the bits of the uncut batch -- the offsets of the frames, of the low
    words of f64 frames, of the minmax table and of both outputs by g0 are all that differs --, on a fresh handle each, and the
    uncut batch must agree with the oracle.  Every group's frames differ from every other's, so no group can stand in for another."""
    cfg, frames, given, yb, kw = _inputs(c, groups=CHUNK_GROUPS, seed=47)
    A, H, W, D = c["A"], c["H"], c["W"], c["D"]
    device = c["name"].startswith("device")
    _group_frames_differ(frames, A)
    batches = [given]
    if c["dtype"] == "f64":
        # ... and once more as doubles that are no floats: the low words are then a plane of their own that differs from group to
        # group (bit-equality only: the oracle's driver takes integer frames)
        frac = given + np.random.default_rng(5).uniform(-0.5, 0.5, given.shape)
        lo = frac - frac.astype(np.float32)
        assert np.count_nonzero(lo) > 0.9 * lo.size
        _group_frames_differ(frac, A, lo)
        batches.append(frac)

    def run(batch, mb):
        if mb is None:
            monkeypatch.delenv("FDOCT_BIG_CHUNK_MB", raising=False)
        else:
            monkeypatch.setenv("FDOCT_BIG_CHUNK_MB", mb)
        r = _handle(c, cfg, yb, kw)
        if not device:
            out = _process_both_layouts(r, c, batch)
        else:
            import torch
            from fdoct_amd import DTYPE_U16
            n, pitch = batch.shape[0], (W + 24) * 2
            d_in = torch.full((n * H, pitch // 2), -1, dtype=torch.int16, device="cuda")
            d_in[:, :W] = torch.from_numpy(batch.view(np.int16).reshape(n * H, W)).cuda()
            d_b = torch.zeros((n // A, H, D), dtype=torch.float32, device="cuda")
            d_d = torch.zeros((n // A, H, D), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r.process_device(d_in.data_ptr(), DTYPE_U16, n, pitch, d_b.data_ptr(), d_d.data_ptr())
            r.synchronize()
            assert r.last_kernel() == capi.KERNEL_LONG_ROWS
            out = d_b.cpu().numpy(), d_d.cpu().numpy()
        r.close()
        return out

    for i, batch in enumerate(batches):
        b, d = run(batch, None)
        for g in range(CHUNK_GROUPS):
            for k in range(g + 1, CHUNK_GROUPS):
                assert not np.array_equal(b[g], b[k]), (g, k)
        for mb in CHUNK_BUDGETS_MB:
            b1, d1 = run(batch, mb)
            np.testing.assert_array_equal(b1, b, err_msg="%s, budget %s MB: magnitudes" % (c["name"], mb))
            np.testing.assert_array_equal(d1, d, err_msg="%s, budget %s MB: dB" % (c["name"], mb))
        if i == 0:
            _hold_to_oracle(c, cfg, frames, yb, kw, b, d, "long rows in chunks, %s" % c["name"])


_PER_PASS_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import test_gpu_long_rows as m
from fdoct_amd import capi
out = {}
for i, c in enumerate(m.PER_PASS_CASES):
    cfg, frames, given, yb, kw = m._inputs(c)
    r = m._handle(c, cfg, yb, kw)
    out["b%d" % i], out["d%d" % i] = m._process_both_layouts(r, c, given)
    r.close()
np.savez(sys.argv[2], **out)
"""


@gpu
def test_one_launch_per_pass_form_in_a_child_process(tmp_path):
    """FDOCT_BIG_PER_PASS=1 (read once per process) runs every transform as one launch of big_fft_pass_kernel per radix, with
    every loader materialised: a fresh interpreter processes a 65610-point case (radices 5, 3 x 8, 2) and a zero-pad case
    (640 -> 2560: radices 5, 8, 4, 2 with the band-pass) and saves the images; they are held to the oracle here."""
    out = tmp_path / "per_pass.npz"
    env = dict(os.environ, FDOCT_BIG_PER_PASS="1")
    env.pop("FDOCT_BIG_CHUNK_MB", None)
    p = subprocess.run([sys.executable, "-c", _PER_PASS_CHILD, ROOT, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    z = np.load(out)
    for i, c in enumerate(PER_PASS_CASES):
        cfg, frames, given, yb, kw = _inputs(c)
        _hold_to_oracle(c, cfg, frames, yb, kw, z["b%d" % i], z["d%d" % i], "long rows, one launch per pass, %s" % c["name"])
