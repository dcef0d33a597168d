"""Device time of the colour front end (include/fdoct_colour.h) on device-resident webcam frames, through the public interface:
256 frames of 640 x 480 x 3 and 32 frames of 1920 x 1080 x 3, channel select (G) and channel sum, bins (1,1) and (2,2).

  trace    the kernels alone: a child under `rocprofv3 --kernel-trace --stats` calls fdoct_colour_extract on device memory and
           the in-tree float4 copy (tools/ubench/copy_f4.hip) in the same process; us per dispatch of colour_vec_kernel and GB/s
           of the bytes it must read and write, next to the copy's rate from the same trace.
  events   the same calls between HIP events on the handle's stream (the call: the kernel plus its packed copy to `out`), and
           the float4 copy likewise.
  process  the whole process_async of a colour handle (640 x 480 set, webcam geometry) against the mono call on the channel
           extracted beforehand, and against the only route without the stage: de-interleave in numpy on the host, upload, mono
           call (wall clock, synchronous, results compared bit for bit).

Every step is a child process of its own under `timeout`; the first one that fails ends the run.  Figures are medians of
`--reps` measurements after a warm-up.

    python3 tools/colour_bench.py [--reps 15] [--out profiles/colour_stage.txt]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = [("640x480", 256, 480, 640), ("1920x1080", 32, 1080, 1920)]
LEGS = [(c, b) for c in (1, 3) for b in ((1, 1), (2, 2))]   # (channelnum, bins), in the order every step runs them
WARMUP = 2
STEP_TIMEOUT = {"trace": 420, "events": 240, "process": 300}


def copy_f4_lib():
    cl = C.CDLL(os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"))
    cl.copy_f4.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    return cl


def stage_bytes(n, h, w, c, bins):
    return n * h * w * 3 + n * (h // bins[1]) * (w // bins[0]) * (8 if c == 3 else 1)


def make_set(n, h, w):
    import numpy as np
    import torch
    t = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def handle(w=640, h=480):
    from fdoct_amd import Config, Reconstructor
    return Reconstructor(Config(width=w, height=h, numfftpoints=640, numdisplaypoints=320))


def event_median(st, fn, reps, inner=4):
    import torch
    for _ in range(WARMUP):
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


def wall_median(fn, reps):
    import torch
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def step_trace_child(reps):
    """Under rocprofv3: the copy, then every set's legs, each WARMUP + reps times."""
    import torch
    cl = copy_f4_lib()
    rec = handle()
    for _, n, h, w in SETS:
        frames = make_set(n, h, w)
        out = torch.empty(n * h * w * 8, dtype=torch.uint8, device="cuda")
        nb = frames.numel() // 16 * 16
        for _ in range(WARMUP + reps):
            assert cl.copy_f4(out.data_ptr(), frames.data_ptr(), nb, 0, 0, None) == 0
        torch.cuda.synchronize()
        for c, bins in LEGS:
            for _ in range(WARMUP + reps):
                rec.colour_extract_device(frames.data_ptr(), n, w, h, 0, c, out.data_ptr(), 0, *bins)
        rec.synchronize()
        del frames, out
    rec.close()


def step_trace(reps, report, keep_in):
    tmp = tempfile.mkdtemp(prefix="colour_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "colour", "--",
               sys.executable, os.path.abspath(__file__), "--step", "trace-child", "--reps", str(reps)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        trace = glob.glob(os.path.join(tmp, "**", "colour_kernel_trace.csv"), recursive=True)[0]
        rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
        dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
        copies = [dur(r) for r in rows if "copy_f4_kernel" in r["Kernel_Name"]]
        stage = [(r["Kernel_Name"], dur(r)) for r in rows if "colour_" in r["Kernel_Name"] and "_kernel" in r["Kernel_Name"]]
        per = WARMUP + reps
        assert len(copies) == per * len(SETS) and len(stage) == per * len(SETS) * len(LEGS), (len(copies), len(stage))
        for si, (name, n, h, w) in enumerate(SETS):
            nb = n * h * w * 3 // 16 * 16
            cus = statistics.median(copies[si * per + WARMUP:(si + 1) * per])
            yard = 2.0 * nb / cus / 1e3
            report(step="trace", op="copy_f4", frames=name, bytes=2 * nb, us=round(cus, 2), gbs=round(yard, 1))
            for li, (c, bins) in enumerate(LEGS):
                k = (si * len(LEGS) + li) * per
                us = statistics.median(d for _, d in stage[k + WARMUP:k + per])
                nbytes = stage_bytes(n, h, w, c, bins)
                report(step="trace", op=(re.search(r"colour_\w+_kernel(<[^>]*>)?", stage[k][0]) or [stage[k][0]])[0], frames=name, channelnum=c, bins=list(bins), bytes=nbytes, us=round(us, 2),
                       gbs=round(nbytes / us / 1e3, 1), of_copy_f4=round(nbytes / us / 1e3 / yard, 3))
        if keep_in:
            for s in glob.glob(os.path.join(tmp, "**", "colour_kernel_stats.csv"), recursive=True)[:1]:
                shutil.copy(s, os.path.join(keep_in, "colour_kernel_stats.csv"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def step_events(reps, report):
    import torch
    st = torch.cuda.Stream()
    cl = copy_f4_lib()
    rec = handle()
    rec.set_stream(st.cuda_stream)
    for name, n, h, w in SETS:
        frames = make_set(n, h, w)
        out = torch.empty(n * h * w * 8, dtype=torch.uint8, device="cuda")
        nb = frames.numel() // 16 * 16
        cus = event_median(st, lambda: cl.copy_f4(out.data_ptr(), frames.data_ptr(), nb, 0, 0, st.cuda_stream), reps)
        yard = 2.0 * nb / cus / 1e3
        report(step="events", op="copy_f4", frames=name, bytes=2 * nb, us=round(cus, 2), gbs=round(yard, 1))
        for c, bins in LEGS:
            us = event_median(st, lambda: rec.colour_extract_device(frames.data_ptr(), n, w, h, 0, c, out.data_ptr(), 0, *bins), reps)
            nbytes = stage_bytes(n, h, w, c, bins)
            report(step="events", op="fdoct_colour_extract (kernel + packed copy to out)", frames=name, channelnum=c, bins=list(bins), bytes=nbytes,
                   us=round(us, 2), gbs=round(nbytes / us / 1e3, 1), of_copy_f4=round(nbytes / us / 1e3 / yard, 3))
        del frames, out
    rec.set_stream(None)
    rec.close()


def step_process(reps, report):
    import numpy as np
    import torch

    import colour_model
    from fdoct_amd import DTYPE_F64, DTYPE_U8, synth
    name, n, h, w = SETS[0]
    st = torch.cuda.Stream()
    host = np.random.default_rng(1).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames = torch.from_numpy(host).cuda()
    mag = torch.empty((n, h, 320), dtype=torch.float32, device="cuda")
    db = torch.empty_like(mag)
    for c in (1, 3):
        colour, mono = handle(), handle()
        for r in (colour, mono):
            r.set_background(synth.make_background(w))
            r.set_stream(st.cuda_stream)
        colour.set_colour_input(c)
        pre = torch.from_numpy(np.ascontiguousarray(colour_model.extract(host, c))).cuda()
        mdt = DTYPE_F64 if c == 3 else DTYPE_U8
        us_c = event_median(st, lambda: colour.process_device(frames.data_ptr(), DTYPE_U8, n, 0, mag.data_ptr(), db.data_ptr()), reps, inner=2)
        got = mag.cpu().numpy()
        us_m = event_median(st, lambda: mono.process_device(pre.data_ptr(), mdt, n, 0, mag.data_ptr(), db.data_ptr()), reps, inner=2)
        same = bool(np.array_equal(got.view(np.uint32), mag.cpu().numpy().view(np.uint32)))
        report(step="process", op="process_async, colour frames", frames=name, channelnum=c, us=round(us_c, 1), ascans_per_s=round(n * h / us_c * 1e6))
        report(step="process", op="process_async, mono handle on the channel extracted beforehand", frames=name, channelnum=c, us=round(us_m, 1),
               ratio_colour_over_mono=round(us_c / us_m, 3), same_bits=same)
        for r in (colour, mono):
            r.set_stream(None)
        out_b, out_d = np.empty((n, h, 320), np.float32), np.empty((n, h, 320), np.float32)
        new_us = wall_median(lambda: colour.process(host, out_bscan=out_b, out_db=out_d), max(3, reps // 3))
        want = out_b.copy()

        def by_hand():
            if c == 3:
                m = (host[..., 0].astype(np.float64) + host[..., 1].astype(np.float64) + host[..., 2].astype(np.float64)) * 0.00130718954
            else:
                m = np.ascontiguousarray(host[..., c])
            mono.process(m, out_bscan=out_b, out_db=out_d)
        old_us = wall_median(by_hand, max(3, reps // 3))
        report(step="process", op="process from host memory, colour frames", frames=name, channelnum=c, us=round(new_us, 1))
        report(step="process", op="by hand: numpy de-interleave on the host, upload, mono call", frames=name, channelnum=c, us=round(old_us, 1),
               ratio_by_hand_over_colour=round(old_us / new_us, 2), same_bits=bool(np.array_equal(want.view(np.uint32), out_b.view(np.uint32))))
        colour.close()
        mono.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: one step, in this process")
    args = ap.parse_args()

    def report(**kw):
        print(json.dumps(kw), flush=True)

    out_dir = os.path.dirname(os.path.abspath(args.out)) if args.out else None
    if args.step == "trace-child":
        return step_trace_child(args.reps)
    if args.step == "trace":
        return step_trace(args.reps, report, out_dir)
    if args.step == "events":
        return step_events(args.reps, report)
    if args.step == "process":
        return step_process(args.reps, report)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    lines = []
    for step in ("trace", "events", "process"):   # chained: a step that fails or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
        if args.out:
            cmd += ["--out", args.out]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit("step %s ended with status %d: nothing further was started" % (step, p.returncode))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/colour_bench.py: device-resident B,G,R frames (%s); us = median of %d measurements\n" %
                    (", ".join("%d x %s" % (n, name) for name, n, _, _ in SETS), args.reps))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
