"""CPU tests of the drop-in boundary: the C-ABI library loads without a GPU, exports every symbol
include/fdoct.h declares, its host-side tables equal the oracle's bit for bit, and it refuses to
compute without a device (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
import fdoct_amd
from fdoct_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "fdoct.h")).read()
    declared = sorted(set(re.findall(r"\b(fdoct_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 20
    lib = fdoct_amd.load_library()
    for name in declared:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(capi.ABI_SYMBOLS) == declared
    assert b"gfx950" in lib.fdoct_version()


@pytest.mark.parametrize("W,M,N", [(128, 1, 1024), (2048, 1, 2048), (4096, 1, 4096), (640, 4, 2560)])
def test_host_tables_equal_oracle_bit_for_bit(W, M, N):
    """fdoct_build_resample_table / fdoct_build_window (product, C++) vs oracle (C): identical doubles."""
    idx, frac = fdoct_amd.build_resample_table(W, M, N, 816e-9, 884e-9)
    oidx, ofrac = orc.tables(W, M, N, 816e-9, 884e-9)
    np.testing.assert_array_equal(idx, oidx)
    np.testing.assert_array_equal(frac, ofrac)
    np.testing.assert_array_equal(fdoct_amd.build_window(W), orc.barthann(W))


def test_create_fails_loudly_without_a_gpu_or_with_bad_config():
    import torch
    cfg = fdoct_amd.Config(width=2048, height=8, numfftpoints=2048, numdisplaypoints=1024)
    if not torch.cuda.is_available():
        with pytest.raises(fdoct_amd.FdoctError) as e:
            fdoct_amd.Reconstructor(cfg)
        assert e.value.code == -3 and "no CPU fallback" in str(e.value)
    lib = fdoct_amd.load_library()
    h = C.c_void_p()
    bad = capi._CConfig(7, 2048, 8, 2048, 1024, 1, 1, 0, 1, 0, 0, 1, 0, 816e-9, 884e-9)  # wrong struct_size
    assert lib.fdoct_create(C.byref(bad), C.byref(h)) == -1
    assert b"struct_size" in lib.fdoct_last_error(None)
    assert lib.fdoct_build_window(1, None) == -1
    # null handle is an error everywhere, never a crash
    assert lib.fdoct_synchronize(None) == -1 and lib.fdoct_set_launch(None, 0, 0) == -1
    assert lib.fdoct_destroy(None) == 0


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    """include/fdoct.h is the boundary a C or C++ host includes: it must compile as C99 (no C++ in the interface), and a
    plain C program must link against libfdoct_hip.so and run its host-only entry points (no GPU needed: the version
    string, the frame-shard rule of fdoct_shard_frames, the k table of BscanFFT.cpp:615-698)."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "fdoct.h"
int main(void) {
  int first = -1, count = -1;
  int32_t idx[1024];
  double frac[1024];
  fdoct_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg;
  if (fdoct_shard_frames(80000, 1, 3, 8, &first, &count) != FDOCT_OK) return 2;
  if (fdoct_build_resample_table(128, 1, 1024, 816e-9, 884e-9, idx, frac) != FDOCT_OK) return 3;
  printf("%s|%d|%d|%d|%d.%d\n", fdoct_version(), first, count, (int)idx[512], FDOCT_VERSION_MAJOR, FDOCT_VERSION_MINOR);
  return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(fdoct_amd.library_path())
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-500:]
    ver, first, count, mid, hv = out.stdout.strip().split("|")
    assert "gfx950" in ver and (int(first), int(count)) == (30000, 10000)     # C5: rank 3 of 8 gets frames 30000..39999
    oidx, _ = orc.tables(128, 1, 1024, 816e-9, 884e-9)
    assert int(mid) == int(oidx[512]) and ver.split()[1].startswith(hv)


def test_out_of_host_memory_in_an_entry_point_is_an_error_code(tmp_path):
    """Nothing throws across the C ABI (include/fdoct.h): tests/native/alloc_fail_check.cpp replaces the global operator new
    so that the k-th allocation fails, and for every k each host-only table builder returns FDOCT_ERR_NOMEM instead of
    taking the process down -- and disarmed computes what it computed before.  Built the way a C++ host links the library."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "alloc_fail_check"
    libdir = os.path.dirname(fdoct_amd.library_path())
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "alloc_fail_check.cpp"), "-o", str(exe),
           "-L", libdir, "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 4, out.stdout


def _native_table(tmp_path, name):
    """Builds tests/native/<name>.cpp the way a C++ host links the library, runs it with the measurement switches of the
    environment off, and returns (printed lines, lines of tests/native/<name>.expected)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / name
    native = os.path.join(ROOT, "tests", "native")
    libdir = os.path.dirname(fdoct_amd.library_path())
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fdoct_amd", "csrc"),
           os.path.join(native, name + ".cpp"), "-o", str(exe),
           "-L", libdir, "-lfdoct_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("FDOCT_")}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines(), open(os.path.join(native, name + ".expected")).read().splitlines()


def test_fused_launch_decisions_match_the_recorded_table(tmp_path):
    """make_fused_launch (fdoct_amd/csrc/fdoct_launch.h) decides, for every handle and call of tests/native/launch_check.cpp's
    grid -- every shape of plan_check.cpp with a fused plan and C1 as stated, with and without a phase; 1 and 16 averages; u8 /
    u16 / f32 samples; one-row and full-frame background; one and both words of the reciprocal; pi frame, dark frame, row-wise
    and whole-frame normalisation, low-word plane, the any-option kernel, staged mode; set_launch overrides of block and grid;
    8 and 262 000 A-scans; the transposed store on 8 / 500 / 1000 rows and 256 / 512 / 1024 depth bins with the ring cap --,
    exactly what launch_check.expected recorded: kernel form, block, LDS, grid, ring and tiles, or the refusal and its text.  The
    table was recorded from the arithmetic moved as it stood in launch_family_fused and fused_transposed_store_applies, before
    their two copies were made one."""
    got, want = _native_table(tmp_path, "launch_check")
    assert len(got) == len(want) and len(want) > 600
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d launches differ, first: %s" % (len(diff), diff[0])


def test_route_decisions_match_the_recorded_table(tmp_path):
    """make_route (fdoct_amd/csrc/fdoct_route_value.h) decides, for every handle and call of tests/native/route_check.cpp's grid --
    a shape of every kind of plan_check.cpp (fused, each built-in wave shape, an EXTRA one, a smooth one off both lists, an odd
    width, a Bluestein length, long rows), three of them crossed with every sample type, reference frame, normalisation, phase, deep display,
    moving average, median, binning (and the in-kernel binning's edges), colour channel, address and pitch off the vector grids,
    layout, staged mode, plan / block / grid override, averaging, one B-scan, jit off, the compiler answering yes and no, and the
    complex call, the others with the options whose launch depends on the shape --, exactly what route_check.expected recorded: the passes in front of the chain, the family, what its kernel
    reads, waves / LDS / grid or the whole fused launch, the table sets, the note, every question put to the run-time compiler
    -- or the refusal and its text, with a line for every pair of refusals that could both apply.  The table was recorded from
    the arithmetic moved as it stood in choose_route_of, before the route became a value.  The program makes no HIP call."""
    got, want = _native_table(tmp_path, "route_check")
    assert len(got) == len(want) and len(want) > 450
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d routes differ, first: %s" % (len(diff), diff[0])
    texts = {l.split(": rc=", 1)[1].split(" |")[0] for l in want if ": rc=" in l}
    assert len(texts) == 13, sorted(texts)   # every refusal of make_route (and one of make_fused_launch's passing through)


def test_plan_decisions_match_the_recorded_table(tmp_path):
    """make_plan (fdoct_amd/csrc/fdoct_plan.h) decides, for every configuration of tests/native/plan_check.cpp's grid -- the
    BASELINE shapes, the shipped ini shapes, odd widths, Bluestein lengths, in-place half lengths, rows beyond the LDS, with and
    without a phase, every plan override, with and without force_general --, exactly what plan_check.expected recorded from the
    planner before the plan was a value: the fused plan and its geometry, or the generic path, and the generic plan."""
    got, want = _native_table(tmp_path, "plan_check")
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d decisions differ, first: %s" % (len(diff), diff[0])


def test_long_row_plans_and_chunks_match_the_recorded_table(tmp_path):
    """The long-row path's host-side decisions (fdoct_amd/csrc/fdoct_big_plan.h) are values without HIP in them.
    tests/native/bigplan_check.cpp asserts their invariants for every length 2^a 3^b 5^c from 2 to 2^24 -- a grouped plan exists,
    the groups' lengths multiply to n and P Q F = n in each, every tile and its LDS fit, the radices multiply to Q, the group
    count is 1 up to 256 points, 2 up to 65 536 and 3 beyond (4 only where three groups cannot hold the factors) -- and for the
    chunks of a batch over a grid of geometries and budgets: 1 <= cg <= G, the chunks cover G exactly, the buffers hold cg A H
    rows; a failed invariant is a non-zero exit status.  Its table -- the plan of every transform length that
    tests/test_gpu_long_rows.py runs and the chunk sequences of its batches -- must equal bigplan_check.expected, recorded from
    big_plan_groups, big_plan_get's radix split and run_big's chunk arithmetic as they were moved out of fdoct_route.cpp."""
    got, want = _native_table(tmp_path, "bigplan_check")
    assert len(got) == len(want) and len(want) > 30
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d rows differ, first: %s" % (len(diff), diff[0])
    assert got[0] == "lengths 2^a 3^b 5^c from 2 to 2^24 checked: 835"


def test_staging_plan_places_host_memory_arguments(tmp_path):
    """The staging plan of the side entry points (fdoct_amd/csrc/fdoct_stage.h) is a value without HIP in it:
    tests/native/stage_check.cpp, built with plain g++ like the two tables above, checks over the plan type alone that every
    staged item starts at a multiple of 256 bytes, that items do not overlap and the totals cover the last one, that device
    items keep the caller's pointer and pitch and add nothing to the totals, that an absent output becomes scratch exactly
    when the kernel writes it anyway, that the in-place pair is one device range, that the 2-D form packs rows to
    (row + 15) & ~15, that the call synchronises exactly when an item is in host memory, and that sizes which would wrap
    size_t are FDOCT_ERR_INVALID."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "stage_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fdoct_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "stage_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout[-2000:] + out.stderr[-2000:]


def test_host_call_decisions_match_the_recorded_table(tmp_path):
    """make_host_call (fdoct_amd/csrc/fdoct_hostcall.h) decides what fdoct_process / fdoct_process_async decide on the host before
    anything is enqueued.  tests/native/hostcall_check.cpp, built with plain g++ against the header alone, prints for its grid --
    2048 x 1000 u16, 1024 x 40 u16, 160 x 120 u8 behind a 2 x 2 front end, 3-byte colour pixels, a frame larger than a chunk;
    1 / 2 / 3 / 16 averages; the sim variant's groups of 1 and 3; every combination of memory spaces; all buffers pinned and one
    pageable, wanted or not; FDOCT_HOST_CHUNK_MB of 0 / 1 / 100000; a padded pitch; nframes at the refusals and on both sides of
    every count at which the decision changes (the legs are listed in the program, not a full cross product) -- every field of
    the value, or the refusal and its text, exactly as
    hostcall_check.expected recorded them.  The order was: the arithmetic moved into the header verbatim from fdoct_process and
    sim_last_frames, the table printed from that and committed, and only then the function restructured.  The rows below are
    derived by hand from the code as it stood (a C2 frame is 4 096 000 bytes; 96 MiB is 24.6 of them)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    native = os.path.join(ROOT, "tests", "native")
    exe = tmp_path / "hostcall_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fdoct_amd", "csrc"),
                        os.path.join(native, "hostcall_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got, want = out.stdout.splitlines(), open(os.path.join(native, "hostcall_check.expected")).read().splitlines()
    assert len(got) == len(want) and len(want) > 600
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d decisions differ, first: %s" % (len(diff), diff[0])

    def row(key):
        (line,) = [l for l in got if l.startswith(key + ": ")]
        words = line[len(key) + 2:].split()
        return words[0], words[1], {k: int(v) for k, v in (x.split("=") for x in words[2:])}

    MB = 1 << 20
    for key, path, chunk, fpc in [("hand: C2 pinned n=3", "single", 8 * MB, 2), ("hand: C2 pinned n=4", "pipelined", 8 * MB, 2),
                                  ("hand: C2 pinned n=24", "pipelined", 8 * MB, 2), ("hand: C2 pinned n=25", "pipelined", 16 * MB, 4),
                                  ("hand: C2 one pageable n=15", "single", 16 * MB, 4), ("hand: C2 one pageable n=16", "pipelined", 16 * MB, 4),
                                  ("hand: C2 A=3 pinned n=3", "single", 8 * MB, 3), ("hand: C2 A=3 pinned n=30", "pipelined", 16 * MB, 3),
                                  ("hand: C2 A=3 pageable n=3", "single", 16 * MB, 3), ("hand: C2 A=3 pageable n=30", "pipelined", 16 * MB, 3)]:
        sim, p, f = row(key)
        assert (sim, p, f["chunk"], f["fpc"]) == ("asis", path, chunk, fpc), key
        assert f["pageable"] == ("pageable" in key) and f["stride"] == 4096000 and f["first"] == 0, key
    for A in (1, 2, 3, 16):  # a frame (32 MiB) above the chunk size: one averaging group per chunk, at both chunk sizes
        for pin in ("pinned", "frames-pageable"):
            f = row("hand: frame above the chunk A=%d %s n=48" % (A, pin))[2]
            assert (f["chunk"], f["fpc"]) == (16 * MB, A)
    for A in (1, 2):  # (two frames are under 96 MiB)
        f = row("4096x4096u16 A=%d S=1 mb=0 h>h pinned n=2" % A)[2]
        assert (f["chunk"], f["fpc"]) == (8 * MB, A)
    sim, p, f = row("hand: sim host>host n=180")
    assert (sim, p) == ("strided", "pipelined")
    assert (f["nframes"], f["fpc"], f["first"], f["stride"], f["chunk"]) == (60, 12, 2 * 81920, 3 * 81920, MB)
    assert row("hand: sim host>device n=180")[:2] == ("gather", "device")


def test_every_entry_point_catches_at_the_boundary():
    """Each extern "C" definition in fdoct_capi.cpp is a function-try-block that ends in the boundary's catch macro
    (FDOCT_CATCH and its variants), and those definitions are exactly the exported ABI."""
    src = open(os.path.join(ROOT, "fdoct_amd", "csrc", "fdoct_capi.cpp")).read()
    body = src[src.index('extern "C" {'):src.rindex('}  // extern "C"')]

    def close_of(i):  # index of the brace that closes the one at i (string / character literals and // comments skipped)
        depth = 0
        while True:
            if body.startswith("//", i):
                i = body.index("\n", i)
                continue
            c = body[i]
            if c in "\"'":
                j = i + 1
                while body[j] != c:
                    j += 2 if body[j] == "\\" else 1
                i = j + 1
                continue
            depth += {"{": 1, "}": -1}.get(c, 0)
            if depth == 0:
                return i
            i += 1

    defined = []
    for m in re.finditer(r"^(?!static\b)[A-Za-z_][\w \*]*?\b(fdoct_\w+)\(", body, re.M):
        head_end = min(k for k in (body.find("{", m.end()), body.find(";", m.end())) if k >= 0)
        if body[head_end] == ";":
            continue  # a declaration
        name = m.group(1)
        defined.append(name)
        assert re.search(r"\)\s*try\s*$", body[m.start():head_end]), name + " is not a function-try-block"
        tail = body[close_of(head_end) + 1:]
        assert re.match(r"\s*FDOCT_CATCH\w*\(", tail), name + " does not end in FDOCT_CATCH"
    assert len(defined) == len(set(defined)) == 50
    assert set(defined) == set(capi.ABI_SYMBOLS)


def test_run_time_compile_of_the_wave_kernel_needs_no_gpu():
    """fdoct_jit_compile_check: the device source that travels inside the library compiles for gfx950 through hipRTC for a
    geometry outside the built-in list (1280 samples, zero-pad x2, numfftpoints 2560), and a geometry the template cannot take
    (half-length transforms with a prime factor above 5) is refused with a reason instead."""
    from fdoct_amd import capi
    n, why = capi.jit_compile_check(1280, 2, 2560, 400)
    assert n > 4096 and why == "", (n, why)
    n, why = capi.jit_compile_check(208, 4, 2560, 320)
    assert n == -1 and "cannot take this shape" in why, (n, why)
    n, why = capi.jit_compile_check(1280, 2, 2560, 400, gcn_arch="gfx000")
    assert n == -1 and why, (n, why)


def opencv_jet_numpy():
    """OpenCV's COLORMAP_JET table restated with numpy float32 arithmetic, step by step as imgproc/src/colormap.cpp builds it:
    Octave's jet(256) rounded to float (the literals of the source), X = linspace(0.f, 1.f, 256), interp1(X, channel, X) in
    float -- low = i - 1, high = i, Y[low] + (X[i] - X[low]) * (Y[high] - Y[low]) / (X[high] - X[low]) --, convertTo(CV_8U, 255.)
    = round-half-even(v * 255.f).  B,G,R."""
    f = np.float32
    i = np.arange(256)
    x = i * (1.0 / 255.0)
    r = ((x >= 3 / 8) & (x < 5 / 8)) * (4 * x - 3 / 2) + ((x >= 5 / 8) & (x < 7 / 8)) + (x >= 7 / 8) * (-4 * x + 9 / 2)
    g = ((x >= 1 / 8) & (x < 3 / 8)) * (4 * x - 1 / 2) + ((x >= 3 / 8) & (x < 5 / 8)) + ((x >= 5 / 8) & (x < 7 / 8)) * (-4 * x + 7 / 2)
    b = (x < 1 / 8) * (4 * x + 1 / 2) + ((x >= 1 / 8) & (x < 3 / 8)) + ((x >= 3 / 8) & (x < 5 / 8)) * (-4 * x + 5 / 2)
    step = f(1.0) / f(255.0)
    X = (f(0.0) + i.astype(f) * step).astype(f)
    out = np.zeros((256, 3), np.uint8)
    for ch, y64 in enumerate((b, g, r)):
        Y = y64.astype(f)
        lut = np.empty(256, f)
        lut[0] = Y[0] + (X[0] - X[0]) * (Y[1] - Y[0]) / (X[1] - X[0])
        lo, hi = slice(0, 255), slice(1, 256)
        num = ((X[hi] - X[lo]) * (Y[hi] - Y[lo])).astype(f)
        lut[1:] = (Y[lo] + (num / (X[hi] - X[lo])).astype(f)).astype(f)
        out[:, ch] = np.clip(np.rint((lut * f(255.0)).astype(f)), 0, 255).astype(np.uint8)     # np.rint: half to even
    return out


def test_builtin_colormap_is_opencv_jet_by_construction():
    """fdoct_build_colormap_jet (C++, float, operation by operation) against the numpy restatement of the same OpenCV recipe,
    the end points every OpenCV build shows, and the structure of the table: every Octave value is (k + 1/2) / 255, so an entry
    is k or k + 1 -- the float roundings decide which, and the two implementations must decide alike."""
    from fdoct_amd.capi import build_colormap_jet
    got = build_colormap_jet()
    want = opencv_jet_numpy()
    np.testing.assert_array_equal(got, want)
    assert tuple(got[0]) == (128, 0, 0) and tuple(got[255]) == (0, 0, 128)            # B,G,R: dark blue .. dark red
    assert (got[96:160, 1] == 255).all() and (got[32:96, 0] == 255).all() and (got[160:224, 2] == 255).all()
    i = np.arange(256)
    rise = 4 * i[96:160] - 382.5                                                       # red on its rising ramp: k + 1/2
    assert np.all((got[96:160, 2] == np.floor(rise)) | (got[96:160, 2] == np.ceil(rise)))
    assert (np.diff(got[96:160, 2].astype(int)) >= 3).all() and (np.diff(got[96:160, 2].astype(int)) <= 5).all()
