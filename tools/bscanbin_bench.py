"""Device time of spinjnt's output binning (include/fdoct_bscanbin.h) through the public interface only, on device-resident C2
output: 262 B-scans of 1000 x 1024 floats, both layouts, both outputs, factors 2 x 2, 3 x 1 (on 999 A-scans) and 4 x 4.

  * bscan_bin_kernel from the kernel trace of a child process (the tool starts itself once more under
    `rocprofv3 --kernel-trace --stats`), and the same launches between HIP events on the handle's stream;
  * against the copy: tools/ubench/copy_f4.hip moving the same number of bytes (input read + both outputs written) between the
    same events, and the call's fraction of it;
  * against the host route, which is what a caller has without the call: download the linear images, the model's arithmetic in
    numpy float64 on the host (tests/bscanbin_model.py, truth mode), upload the dB -- timed on `--host-bscans` B-scans and scaled;
  * the call's share of a C2 step: fdoct_process_async on 262 frames timed next to it.

Every figure is the median of `--reps` measurements after a warm-up.

    python3 tools/bscanbin_bench.py [--reps 9] [--out profiles/bscanbin_bench.txt]
"""
import argparse
import csv
import ctypes
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdoct_amd import DTYPE_U16, LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED, Config, Reconstructor, capi, synth  # noqa: E402

W, H, N, D, G = 2048, 1000, 2048, 1024, 262
CASES = [(2, 2, 1000), (3, 1, 999), (4, 4, 1000)]     # binx, biny, A-scans used (3 does not divide 1000)
LAYOUTS = [("D x H", LAYOUT_TRANSPOSED), ("row-major", LAYOUT_ROWMAJOR)]
TRACE_WARMUP = 2


def device_bscans(ascans):
    """G linear B-scans with reflector peaks on a floor (the values do not change the kernel's work)."""
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.uniform(0.5, 1.5, (G, D * ascans)).astype(np.float32)).cuda()
    x[:, ::997] += 2000.0
    torch.cuda.synchronize()
    return x


def legs():
    for binx, biny, ascans in CASES:
        for lname, layout in LAYOUTS:
            yield binx, biny, ascans, lname, layout


def trace_leg(reps):
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    for binx, biny, ascans, _, layout in legs():
        x = device_bscans(ascans)
        lin, db = torch.empty_like(x), torch.empty_like(x)
        for _ in range(TRACE_WARMUP + reps):
            rec.bscan_bin_device(x.data_ptr(), G, D, ascans, binx, biny, lin.data_ptr(), db.data_ptr(), layout=layout)
        rec.synchronize()
        del x, lin, db
    rec.close()


def kernel_legs_from_trace(reps):
    tmp = tempfile.mkdtemp(prefix="bscanbin_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "bscanbin", "--",
               sys.executable, os.path.abspath(__file__), "--trace-leg", "--reps", str(reps)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        trace = glob.glob(os.path.join(tmp, "**", "bscanbin_kernel_trace.csv"), recursive=True)[0]
        rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
        durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "bscan_bin_kernel" in r["Kernel_Name"]]
        per = TRACE_WARMUP + reps
        keys = [(b, c, l) for b, c, _, l, _ in legs()]
        assert len(durs) == per * len(keys), len(durs)
        return {k: statistics.median(durs[i * per + TRACE_WARMUP:(i + 1) * per]) for i, k in enumerate(keys)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def event_median(st, fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-bscans", type=int, default=4)
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

    traced = kernel_legs_from_trace(args.reps)   # before this process opens the GPU
    import bscanbin_model
    cl = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"))
    cl.copy_f4.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    st = torch.cuda.Stream()
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(synth.make_background(W))
    rec.set_stream(st.cuda_stream)
    # a C2 step next to it: 262 frames through the chain, dB only, device memory
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 65536, (G, H, W), dtype=np.uint16).view(np.int16)).cuda()
    chain_db = torch.empty(G, H, D, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    step_us = event_median(st, lambda: rec.process_device(frames.data_ptr(), DTYPE_U16, G, 0, None, chain_db.data_ptr()), args.reps)
    report(op="fdoct_process_async, C2 step of 262 frames (u16 in, dB out, row-major)", us=round(step_us, 1))
    del frames, chain_db
    for binx, biny, ascans, lname, layout in legs():
        x = device_bscans(ascans)
        lin, db = torch.empty_like(x), torch.empty_like(x)
        us = event_median(st, lambda: rec.bscan_bin_device(x.data_ptr(), G, D, ascans, binx, biny, lin.data_ptr(), db.data_ptr(), layout=layout), args.reps)
        nbytes = 3 * x.numel() * 4            # input read + two outputs written
        half = nbytes // 2 // 16 * 16         # the copy reads and writes: half the bytes each way
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        copy_us = event_median(st, lambda: cl.copy_f4(dst.data_ptr(), src.data_ptr(), half, 0, 0, st.cuda_stream), args.reps)
        del src, dst
        k_us = traced[(binx, biny, lname)]
        report(op="fdoct_bscan_bin", bin="%dx%d" % (binx, biny), layout=lname, bscans=G, image="%d x %d" % (D, ascans),
               kernel_trace_us=round(k_us, 1), hip_events_us=round(us, 1), mbytes_moved=round(nbytes / 1e6, 1),
               gbs=round(nbytes / k_us / 1e3, 1), copy_f4_same_bytes_us=round(copy_us, 1), fraction_of_copy=round(copy_us / k_us, 3),
               share_of_c2_step=round(k_us / step_us, 3))
        if layout == LAYOUT_TRANSPOSED:   # the host route on a few B-scans, scaled to the batch
            nb = args.host_bscans
            pics = x[:nb].view(nb, D, ascans)

            def host_route():
                h = pics.cpu().numpy()
                out = np.stack([bscanbin_model.bscan_bin(p, binx, biny)[1] for p in h]).astype(np.float32)
                return torch.from_numpy(out).cuda()
            host_route()
            t = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = host_route()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e6)
            same = bool(torch.equal(got.view(nb, -1), db[:nb]))
            host_us = statistics.median(t) * G / nb
            report(op="host route: download, numpy float64 model, upload the dB", bin="%dx%d" % (binx, biny), timed_bscans=nb,
                   scaled_to_bscans=G, us=round(host_us, 1), ratio_host_over_library=round(host_us / us, 1), same_db_bits=same)
        del x, lin, db
    rec.set_stream(None)
    rec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/bscanbin_bench.py: 262 device-resident B-scans, both outputs; us = median of %d measurements\n" % args.reps)
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
