"""tests/option_pairs.py held to its conditions on the CPU, with the reference alone: the covering property recomputed by brute
force over the constraint predicates, independently of the generator; determinism; every case admissible; every expected kernel
inside its family's set and equal to what make_route decides for the call (tests/native/option_pairs_route.cpp, the run-time
compiler answering yes); and the oracle condition -- on every case but the band-pass ones the f32 restatement lies within
resample_tables.ORACLE_LIMIT of the chain in double, so that on the GPU the 0.5 of helpers.TRUTH_LIMIT governs."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fdoct_amd
import option_pairs as op
import resample_tables as rt
from fdoct_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _admissible_pairs(fam):
    """Every pair of levels of two options that some admissible case holds, by brute force: the product of the family's levels of
    every option a constraint reads, each predicate given the options of its scope and nothing else; an option no constraint reads
    is free."""
    levels = {f: fam.levels.get(f, (op.DEFAULT[f],)) for f in op.NAMES}
    bound = [f for f in op.NAMES if any(f in k.scope for k in op.CONSTRAINTS)]
    good = [dict(zip(bound, lv)) for lv in itertools.product(*(levels[f] for f in bound))]
    good = [c for c in good if all(k.pred(fam, {s: c[s] for s in k.scope}) for k in op.CONSTRAINTS)]
    pairs = set()
    for a, b in itertools.combinations(op.NAMES, 2):
        for la, lb in itertools.product(levels[a], levels[b]):
            if any(all(c[f] == lv for f, lv in ((a, la), (b, lb)) if f in c) for c in good):
                pairs.add(((a, la), (b, lb)))
    return pairs


@pytest.mark.parametrize("name", op.FAMILY_IDS)
def test_every_admissible_pair_of_levels_is_held_by_a_case(name):
    fam = op.family(name)
    cases = op.generate(name)
    want = _admissible_pairs(fam)
    got = set().union(*(op.pairs_of(c) for c in cases))
    uncovered = {p for p, _ in op.UNCOVERED_PAIRS.get(name, ())}
    print("%s: %d cases, %d admissible pairs, %d uncovered" % (name, len(cases), len(want), len(uncovered)))
    assert got <= want, "cases hold pairs the constraints refuse: %s" % sorted(got - want)[:3]
    assert want - got == uncovered, "pairs no case holds: %s" % sorted(want - got)[:5]
    assert len(uncovered) <= 0.02 * len(want)
    # the aim; coverage wins where a family needs more (none does)
    assert len(cases) <= op.TARGET, len(cases)


def test_the_generator_is_deterministic():
    for name in op.FAMILY_IDS[:3] + op.FAMILY_IDS[-2:]:
        again = op.generate.__wrapped__(name)
        assert again == op.generate(name), name
    assert op.generate.__wrapped__(op.FAMILY_IDS[0], seed=op.SEED + 1) != op.generate(op.FAMILY_IDS[0])


@pytest.mark.parametrize("name", op.FAMILY_IDS)
def test_every_case_is_admissible_and_names_a_kernel_of_its_family(name):
    fam = op.family(name)
    cases = op.generate(name)
    assert len(set(cases)) == len(cases)
    ids = [op.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids)
    for c in cases:
        assert op.admissible(fam, c), c
        assert op.expected_kernel(fam, c) in fam.kernels, c
        assert not (c.samples == "f64" and op.f64_integer(c))
    # every kernel the family can reach is reached
    assert {op.expected_kernel(fam, c) for c in cases} == set(fam.kernels), name
    # the joint the row-independence test of tests/test_gpu_option_pairs.py needs
    c = op.row_independence_case(name)
    assert c is not None and c.averages > 1
    base = {f: fam.levels.get(f, (op.DEFAULT[f],))[0] for f in op.NAMES}
    if any(op.admissible(fam, dict(base, norm="whole", averages=a)) for a in (2, 3)):
        assert c.norm == "whole"


def test_constraints_read_their_scope_only():
    """What _admissible_pairs relies on: a predicate given its scope alone answers as it does on the whole case."""
    for name in op.FAMILY_IDS:
        fam = op.family(name)
        for c in op.generate(name):
            d = c._asdict()
            for k in op.CONSTRAINTS:
                assert k.pred(fam, {s: d[s] for s in k.scope}) == k.pred(fam, d)


def test_expected_kernels_are_what_make_route_decides(tmp_path):
    """Every case as a call of make_route (fdoct_amd/csrc/fdoct_route_value.h), built the way a C++ host links the library: the
    family the decision names is the catalogue's expected kernel, no call is refused, and a D x H image outside the store's set
    comes from the transpose pass."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "option_pairs_route"
    libdir = os.path.dirname(fdoct_amd.library_path())
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fdoct_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "option_pairs_route.cpp"), "-o", str(exe),
           "-L", libdir, "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = [(name, c) for name in op.FAMILY_IDS for c in op.generate(name)]
    lines = tmp_path / "calls.txt"
    lines.write_text("".join(" ".join(str(int(v)) for v in op.route_line(op.family(n), c)) + "\n" for n, c in calls))
    env = {k: v for k, v in os.environ.items() if not k.startswith("FDOCT_")}
    out = subprocess.run([str(exe), str(lines)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(calls)
    bad = []
    for (name, c), line in zip(calls, got):
        fam = op.family(name)
        want = str(op.expected_kernel(fam, c))
        tr = c.layout == "DxH" and op.expected_kernel(fam, c) != capi.KERNEL_FUSED_TRANSPOSED
        if line.split(" opt=")[0] != want + (" tr" if tr else ""):
            bad.append("%s, %s: expected %s, make_route says %s" % (name, op.case_id(c), want, line))
    assert not bad, "%d of %d:\n  " % (len(bad), len(calls)) + "\n  ".join(bad[:20])


@pytest.mark.parametrize("name", op.FAMILY_IDS)
def test_the_f32_restatement_leaves_room_on_every_case(name):
    """The oracle condition.  Band-pass cases are exempt: on short rows the float chain is itself far from its mathematics (DESIGN
    section 4); on the GPU they are held to the chain in double alone."""
    cases = op.generate(name)
    worst, misses = 0.0, []
    for n, c in enumerate(cases):
        mag_o, db_o, mag_t, db_t = op.reference(name, c)
        assert all(np.isfinite(a).all() for a in (mag_o, db_o, mag_t, db_t)), c
        if c.bandpass == "on":
            continue
        o = op.oracle_distance(name, c)
        worst = max(worst, o)
        if o > rt.ORACLE_LIMIT:
            misses.append("case %d (%s): %.3g" % (n, op.case_id(c), o))
    print("%s: %d cases, worst f32 oracle / truth = %.3g" % (name, len(cases), worst))
    assert not misses, "beyond %.2g x the tolerance: %s" % (rt.ORACLE_LIMIT, "; ".join(misses))
