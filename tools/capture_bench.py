"""Device time of the reference-frame capture (include/fdoct_capture.h) on C2 camera frames (2048 x 1000 u16, device-resident),
through the public interface only:

  * capture_accumulate_kernel alone, 16 and 262 frames, movavgn 0 and 3: the tool starts itself once more under
    `rocprofv3 --kernel-trace --stats`; that child calls fdoct_capture_reference(FDOCT_REF_NONE) repeatedly and the in-tree
    float4 copy (tools/ubench/copy_f4.hip, 1 GiB device to device) in the same process, and the kernels' durations are read
    from its trace: us per dispatch and GB/s of the bytes the kernel must read and write (nframes x 4 MB in, 16 MB of doubles
    out), next to the copy's rate from the same trace;
  * fdoct_frame_minmax on 262 frames, device results, and the float4 copy again: HIP events on the handle's stream;
  * the whole fdoct_capture_reference(BACKGROUND) call on 16 device frames (wall clock: it is synchronous and ends with the
    doubles on the host) against what a caller had to do without it for the same result: copy the 16 frames to pageable host
    memory, accumulate in float64 and divide in numpy, fdoct_set_background.  The two results are compared bit for bit.

Every figure is the median of `--reps` measurements after a warm-up.

    python3 tools/capture_bench.py [--reps 15] [--out profiles/capture_bench.txt]
(--out also keeps the child's per-kernel totals next to it as capture_kernel_stats.csv)
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdoct_amd import DTYPE_U16, REF_BACKGROUND, REF_NONE, Config, Reconstructor  # noqa: E402

W, H, N, D = 2048, 1000, 2048, 1024
FRAME_BYTES = W * H * 2


TRACE_WARMUP = 2                                    # dispatches of every leg the trace reader drops
TRACE_LEGS = [(0, 16), (0, 262), (3, 16), (3, 262)]  # (movavgn, nframes), in the order the child runs them


def copy_f4_lib():
    cl = C.CDLL(os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"))
    cl.copy_f4.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    return cl


def make_frames(n):
    rng = np.random.default_rng(1)
    t = torch.from_numpy(rng.integers(0, 65536, (n, H, W), dtype=np.uint16).view(np.int16)).cuda()
    torch.cuda.synchronize()
    return t


def trace_leg(reps):
    """The child under rocprofv3: the copy, then every leg's captures, each TRACE_WARMUP + reps times, in TRACE_LEGS' order."""
    frames = make_frames(262)
    src = frames.view(torch.uint8).reshape(-1)
    nb = min(src.numel(), 1 << 30) // 16 * 16
    dst = torch.empty(nb, dtype=torch.uint8, device="cuda")
    cl = copy_f4_lib()
    for _ in range(TRACE_WARMUP + reps):
        assert cl.copy_f4(dst.data_ptr(), src.data_ptr(), nb, 0, 0, None) == 0
    torch.cuda.synchronize()
    del dst
    for mov in sorted({m for m, _ in TRACE_LEGS}):
        rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, movavgn=mov))
        for m, nframes in TRACE_LEGS:
            if m == mov:
                for _ in range(TRACE_WARMUP + reps):
                    rec.capture_reference_device(REF_NONE, frames.data_ptr(), DTYPE_U16, nframes, 0)
        rec.close()
    print(json.dumps({"copy_bytes": nb}), flush=True)


def kernel_legs_from_trace(reps, keep_stats_in=None):
    """Runs trace_leg in a fresh process under rocprofv3 and returns (copy us, copy bytes, {leg: us}) from its kernel trace."""
    tmp = tempfile.mkdtemp(prefix="capture_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "capture", "--",
               sys.executable, os.path.abspath(__file__), "--trace-leg", "--reps", str(reps)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        nb = [json.loads(ln)["copy_bytes"] for ln in out.stdout.splitlines() if ln.startswith('{"copy_bytes"')][0]
        trace = glob.glob(os.path.join(tmp, "**", "capture_kernel_trace.csv"), recursive=True)[0]
        rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
        dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
        copies = [dur(r) for r in rows if "copy_f4_kernel" in r["Kernel_Name"]]
        caps = [dur(r) for r in rows if "capture_accumulate_kernel" in r["Kernel_Name"]]
        per = TRACE_WARMUP + reps
        assert len(copies) == per and len(caps) == per * len(TRACE_LEGS), (len(copies), len(caps))
        legs = {leg: statistics.median(caps[i * per + TRACE_WARMUP:(i + 1) * per]) for i, leg in enumerate(TRACE_LEGS)}
        if keep_stats_in:
            stats = glob.glob(os.path.join(tmp, "**", "capture_kernel_stats.csv"), recursive=True)
            if stats:
                shutil.copy(stats[0], os.path.join(keep_stats_in, "capture_kernel_stats.csv"))
        return statistics.median(copies[TRACE_WARMUP:]), nb, legs
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def event_median(st, fn, reps, inner=4, warmup=3):
    """Median over `reps` of the us per call of `inner` back-to-back calls between two events."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(inner):
            fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(out)


def wall_median(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-leg", action="store_true", help="internal: the part that runs under rocprofv3")
    args = ap.parse_args()
    if args.trace_leg:
        trace_leg(args.reps)
        return
    lines = []

    def report(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    # the kernel alone, from the trace of a child process (before this process opens the GPU)
    out_dir = os.path.dirname(os.path.abspath(args.out)) if args.out else None
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    copy_us, copy_bytes, legs = kernel_legs_from_trace(args.reps, out_dir)
    yard_trace = 2.0 * copy_bytes / copy_us / 1e3
    report(op="copy_f4", how="kernel trace", bytes=copy_bytes, us=round(copy_us, 2), gbs=round(yard_trace, 1))
    for (mov, nframes), us in legs.items():
        nbytes = nframes * FRAME_BYTES + H * W * 8
        report(op="capture_accumulate_kernel", how="kernel trace", nframes=nframes, movavgn=mov, us=round(us, 2),
               gbs=round(nbytes / us / 1e3, 1), of_copy_f4=round(nbytes / us / 1e3 / yard_trace, 3))

    st = torch.cuda.Stream()
    nmax = 262
    frames = make_frames(nmax)
    res = torch.empty(2 * nmax, dtype=torch.float64, device="cuda")
    cl = copy_f4_lib()
    src = frames.view(torch.uint8).reshape(-1)
    nb = min(src.numel(), 1 << 30) // 16 * 16
    dst = torch.empty(nb, dtype=torch.uint8, device="cuda")
    copy_gbs = {}
    for vname, variant in (("plain", 0), ("nontemporal", 1)):
        us = event_median(st, lambda: cl.copy_f4(dst.data_ptr(), src.data_ptr(), nb, variant, 0, st.cuda_stream), args.reps)
        copy_gbs[vname] = 2.0 * nb / us / 1e3
        report(op="copy_f4", how="HIP events", variant=vname, bytes=nb, us=round(us, 2), gbs=round(copy_gbs[vname], 1))
    yard = max(copy_gbs.values())
    del dst

    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_stream(st.cuda_stream)
    us = event_median(st, lambda: rec.frame_minmax_device(frames.data_ptr(), DTYPE_U16, nmax, 0, res.data_ptr(), res.data_ptr() + 8 * nmax),
                      args.reps)
    nbytes = nmax * FRAME_BYTES
    report(op="fdoct_frame_minmax", how="HIP events", nframes=nmax, us=round(us, 2), gbs=round(nbytes / us / 1e3, 1), of_copy_f4=round(nbytes / us / 1e3 / yard, 3))
    rec.set_stream(None)

    # the whole call against the caller's own recipe
    n = 16
    new_us = wall_median(lambda: rec.capture_reference_device(REF_BACKGROUND, frames.data_ptr(), DTYPE_U16, n, 0), args.reps)
    captured = rec.get_reference(REF_BACKGROUND)

    def by_hand():
        host = frames[:n].cpu().numpy().view(np.uint16)   # hipMemcpy to pageable host memory
        a = np.zeros((H, W), np.float64)
        for f in host:                                    # accumulate(data_y, baccum), frame by frame
            a += f
        a /= float(n)
        rec.set_background(a)
    old_us = wall_median(by_hand, args.reps)
    same = bool(np.array_equal(rec.get_reference(REF_BACKGROUND).view(np.uint64), captured.view(np.uint64)))
    report(op="fdoct_capture_reference(BACKGROUND), 16 device frames, whole call", us=round(new_us, 1))
    report(op="by hand: copy 16 frames to pageable host memory, numpy float64 accumulate and divide, fdoct_set_background",
           us=round(old_us, 1), ratio_by_hand_over_capture=round(old_us / new_us, 2), same_bits=same)
    rec.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/capture_bench.py: C2 camera frames (%d x %d u16, device-resident); us = median of %d measurements\n" % (W, H, args.reps))
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
