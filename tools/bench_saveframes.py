"""What per-frame saves cost over plain averaging (include/fdoct_saveframes.h), through the public interface only, for C2's shape:
64 device-resident u16 frames of 2048 samples x 1000 lines, numfftpoints 2048, numdisplaypoints 1024, averages 16.

  averaged   the averaged chain alone: fdoct_process_async with averages = 16, D x H bscan and bscandb out.  With --parent-root
             the step imports the package of THAT tree (a built checkout of the parent commit), so the figure is the chain
             before the raw-magnitudes switch existed.
  route      the new route: fdoct_process_async with averages = 1 and raw magnitudes on (H x D magnitudes of every frame),
             then fdoct_saveframes on them where they lie, fold (D x H bscan and bscandb) and 64 pictures.  The chain, the
             stage and the two back to back.
  stage      the stage alone as bytes over time -- nframes * H * D * 5 + the fold's output -- against
             tools/ubench/copy_f4.hip moving the same number of bytes, in the same process on the same card, the two alternating.
             The picture pass reads every image a second time; whether that read comes from cache shows in how far the stage
             sits below the copy.

Without --step this is the driver: it runs the three steps as processes of their own, each under its own `timeout -k 10`,
chained with &&, and writes their JSON lines to --out.  Each measurement is `--calls` launches back to back between two HIP
events on the handle's stream, divided by their number; every figure is the median of `--reps` measurements after a warm-up.

    python3 tools/bench_saveframes.py [--parent-root DIR] [--reps 9] [--calls 5] [--out profiles/bench_saveframes.txt]
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, D, A, NF = 2048, 1000, 2048, 1024, 16, 64
STEP_SECONDS = {"averaged": 120, "route": 120, "stage": 120}


def event_median(torch, st, fn, calls, reps, warmup=2):
    out = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(calls):
            fn()
        b.record(st)
        b.synchronize()
        if r >= warmup:
            out.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(out)


def step(name, args):
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    import numpy as np
    import torch
    from fdoct_amd import Config, Reconstructor, capi, synth
    st = torch.cuda.Stream()
    distinct = synth.make_frames(0, 8, W, H)
    frames = torch.from_numpy(np.tile(distinct, (NF // 8, 1, 1)).view(np.int16)).cuda()
    G, px = NF // A, H * D
    res = dict(step=name, frames=NF, shape="%d x %d" % (H, D), averages=A, device=torch.cuda.get_device_name(0),
               library=os.path.relpath(capi.library_path(), ROOT), version=capi.load_library().fdoct_version().decode())

    def handle(averages, raw):
        r = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, averages=averages))
        r.set_background(synth.make_background(W))
        r.set_stream(st.cuda_stream)
        if raw:
            r.set_raw_magnitudes(True)
        return r

    b, db = torch.empty((G, D, H), dtype=torch.float32, device="cuda"), torch.empty((G, D, H), dtype=torch.float32, device="cuda")
    if name == "averaged":
        r = handle(A, False)
        res["averaged_chain_us"] = round(event_median(torch, st, lambda: r.process_device(
            frames.data_ptr(), capi.DTYPE_U16, NF, 0, b.data_ptr(), db.data_ptr(), capi.LAYOUT_TRANSPOSED), args.calls, args.reps), 1)
        res["kernel"] = r.last_kernel()
    else:
        r = handle(1, True)
        mag = torch.empty((NF, H, D), dtype=torch.float32, device="cuda")
        gray = torch.empty((NF, D, H), dtype=torch.uint8, device="cuda")

        def chain():
            r.process_device(frames.data_ptr(), capi.DTYPE_U16, NF, 0, mag.data_ptr(), None, capi.LAYOUT_ROWMAJOR)

        def stage():
            r.saveframes_device(mag.data_ptr(), NF, D, H, gray.data_ptr(), A, b.data_ptr(), db.data_ptr(), capi.LAYOUT_ROWMAJOR,
                                capi.LAYOUT_TRANSPOSED)

        chain()
        if name == "route":
            res["chain_raw_a1_us"] = round(event_median(torch, st, chain, args.calls, args.reps), 1)
            res["saveframes_us"] = round(event_median(torch, st, stage, args.calls, args.reps), 1)
            res["route_us"] = round(event_median(torch, st, lambda: (chain(), stage()), args.calls, args.reps), 1)
            res["kernel"] = r.last_kernel()
        else:
            import ctypes
            cl = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"))
            cl.copy_f4.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
            nbytes = NF * px * 5 + 2 * G * px * 4
            half = nbytes // 2 // 16 * 16          # the copy reads and writes: half the bytes each way
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rows = []
            for _ in range(3):                      # the two alternate, so that a drift of the clock shows in both
                rows.append((event_median(torch, st, stage, args.calls, args.reps),
                             event_median(torch, st, lambda: cl.copy_f4(dst.data_ptr(), src.data_ptr(), half, 0, 0, st.cuda_stream),
                                          args.calls, args.reps)))
            s_us, c_us = statistics.median(x[0] for x in rows), statistics.median(x[1] for x in rows)
            res.update(mbytes=round(nbytes / 1e6, 1), saveframes_us=round(s_us, 1), saveframes_gbs=round(nbytes / s_us / 1e3, 1),
                       copy_f4_same_bytes_us=round(c_us, 1), copy_gbs=round(2 * half / c_us / 1e3, 1),
                       fraction_of_copy=round(c_us / s_us, 3), rounds=[[round(x, 1), round(y, 1)] for x, y in rows])
    torch.cuda.synchronize()
    r.set_stream(None)
    r.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None)
    ap.add_argument("--root", default=None, help="with --step: the tree whose fdoct_amd package the step imports (default: this one)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit for the `averaged` step")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    me = "%s %s --reps %d --calls %d" % (shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)), args.reps, args.calls)
    parts = []
    for name in ("averaged", "route", "stage"):
        root = " --root %s" % shlex.quote(os.path.abspath(args.parent_root)) if name == "averaged" and args.parent_root else ""
        parts.append("timeout -k 10 %d %s --step %s%s" % (STEP_SECONDS[name], me, name, root))
    out = subprocess.run(["bash", "-c", " && ".join(parts)], capture_output=True, text=True)
    sys.stdout.write(out.stdout)
    sys.stderr.write(out.stderr[-4000:])
    if args.out and out.returncode == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/bench_saveframes.py: us per call = median of %d measurements of %d calls back to back, HIP events\n" % (args.reps, args.calls))
            f.write(out.stdout)
    return out.returncode


if __name__ == "__main__":
    sys.exit(main())
