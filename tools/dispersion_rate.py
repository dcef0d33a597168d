"""Transforms per second of the dispersion search (fdoct_dispersion_search, include/fdoct_dispersion.h) on device-resident complex
A-scans, through the public interface only:

  a 64 x 64 grid (K = 4096 candidates) over 64 A-scans of n = 1024, 2048 and 4096 points -- 2.6 x 10^5
  inverse transforms a call -- with the plan's own chunk.  transforms = rows x K, the inverse transforms the result needs; the
  forward transforms the chunking repeats (rows x chunks) are overhead and are not counted.
  Next to each, the comparison point: the workgroup-per-row kernel's complex rate on the same n -- process_complex_device on a handle
  of width n, numfftpoints = numdisplaypoints = n, 1000 rows, 16 frames, run-time compilation off so that the family is that one --
  in A-scans per second: one transform of n points each, with the rest of the chain (u16 load, background, resample, window)
  around it.

  --sweep C1,C2,...: the same search with FDOCT_DISPERSION_CHUNK set to each value (the library reads the switch once, so every
  value runs in a child process of its own, one after the other), on n = 2048: what the chunk rule was chosen from.

Times are device events on the stream the handle is given, around each call: the median of --reps launches after --warmup.

    python3 tools/dispersion_rate.py [--reps 20] [--warmup 3] [--sweep 1,2,4,8,16,32,64,128,512] [--append profiles/dispersion_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, A2, A3 = 64, (-32.0, 1.0, 64), (-16.0, 0.5, 64)


def timed(fn, reps, warmup, stream):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for it in range(warmup + reps):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def search_line(n, reps, warmup, chunk=None):
    import numpy as np
    import torch
    from fdoct_amd import Config, Reconstructor, dispersion
    stream = torch.cuda.current_stream()
    rec = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage reads nothing of the geometry
    rec.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(0)
    X = (rng.normal(0, 1e3, (ROWS, n)) + 1j * rng.normal(0, 1e3, (ROWS, n))).astype(np.complex64)
    d_x = torch.from_numpy(X.view(np.float32).reshape(-1)).cuda()
    p = dispersion.plan(A2, A3, ROWS, n, (2, 0))
    K = p["candidates"]
    d_sums = torch.empty(K * 2, dtype=torch.float64, device="cuda")
    d_rows = torch.empty(ROWS * K * 2, dtype=torch.float64, device="cuda")
    d_best = torch.empty(5, dtype=torch.float64, device="cuda")
    d_tab = torch.empty(n * 2, dtype=torch.float32, device="cuda")
    ms = timed(lambda: dispersion.search_device(rec, d_x.data_ptr(), ROWS, n, A2, A3, d_sums.data_ptr(), d_rows.data_ptr(), d_best.data_ptr(),
                                                d_tab.data_ptr(), depth=(2, 0)), reps, warmup, stream)
    rec.close()
    med = statistics.median(ms)
    return dict(what="search, 64 x 64 candidates, 64 A-scans", n=n, per_workgroup=p["per_workgroup"], chunks=p["chunks"], workgroups=p["workgroups"],
                lds_bytes=p["lds_bytes"], chunk_forced=chunk, ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms),
                transforms=ROWS * K, transforms_per_s=round(ROWS * K / (med * 1e-3), 0), forward_transforms_repeated=ROWS * p["chunks"])


def chain_line(n, reps, warmup):
    import numpy as np
    import torch
    from fdoct_amd import Config, Reconstructor, capi, synth
    stream = torch.cuda.current_stream()
    H, nframes = 1000, 16
    rec = Reconstructor(Config(width=n, height=H, numfftpoints=n, numdisplaypoints=n))
    rec.set_background(synth.make_background(n))
    rec.set_jit(False)
    rec.set_stream(stream.cuda_stream)
    base = synth.make_frames(0, 2, n, H)
    frames = np.ascontiguousarray(base[np.arange(nframes) % 2])
    d_fr = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
    d_cx = torch.empty(nframes * H * n * 2, dtype=torch.float32, device="cuda")
    ms = timed(lambda: rec.process_complex_device(d_fr.data_ptr(), capi.DTYPE_U16, nframes, 2 * n, d_cx.data_ptr()), reps, warmup, stream)
    kernel = rec.last_kernel()
    rec.close()
    med = statistics.median(ms)
    return dict(what="process_complex, workgroup-per-row kernel, %d x %d A-scans" % (nframes, H), n=n, chain_kernel=kernel, ms=round(med, 4),
                min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms), ascans_per_s=round(nframes * H / (med * 1e-3), 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--child-chunk", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 timed launches")
    import torch
    from fdoct_amd import FdoctError
    lines = []
    if args.child_chunk:   # one value of the sweep: the switch is in the environment already
        with torch.cuda.stream(torch.cuda.Stream()):
            print(json.dumps(search_line(2048, args.reps, args.warmup, chunk=args.child_chunk)), flush=True)
        return
    with torch.cuda.stream(torch.cuda.Stream()):
        for n in (1024, 2048, 4096):
            lines.append(search_line(n, args.reps, args.warmup))
            try:
                lines.append(chain_line(n, args.reps, args.warmup))
            except FdoctError as e:
                lines.append(dict(what="process_complex, workgroup-per-row kernel", n=n, note="refused: %s" % e))
        torch.cuda.synchronize()
    for c in [int(v) for v in args.sweep.split(",") if v]:
        env = dict(os.environ, FDOCT_DISPERSION_CHUNK=str(c))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-chunk", str(c), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit("the sweep's child for chunk %d failed (%d): %s" % (c, r.returncode, r.stderr[-2000:]))
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/dispersion_rate.py: the dispersion search on 64 device-resident A-scans, 64 x 64 candidates; transforms = rows x K "
                        "inverse transforms; ms = median of device events over `launches` calls; beside it process_complex on the workgroup-per-row "
                        "kernel at the same n; lines with chunk_forced: FDOCT_DISPERSION_CHUNK, n = 2048\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
