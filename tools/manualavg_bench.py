"""Device time of manual averaging (include/fdoct_manualavg.h) through the public interface only: fdoct_manualavg_add on 64
device-resident images of 1024 x 1000 floats, manualaverages 7, the reference's mode (8 emissions per call, the counter back at 0
after every call), both outputs in device memory -- against tools/ubench/copy_f4.hip moving the same number of bytes, in the same
process on the same card, the two alternating.

Bytes of a call: every input byte once, every emitted byte once (two outputs) and 16 bytes of accumulator per element.  (The
kernel does not fetch the images the mode drops, 8 of the 64 here; the figure counts them, so it is a lower bound on the time
per byte actually moved.)  Each measurement is `--calls` launches back to back between two HIP events on the handle's stream,
divided by their number; every figure is the median of `--reps` measurements after a warm-up.

    python3 tools/manualavg_bench.py [--reps 9] [--calls 10] [--out profiles/manualavg_bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdoct_amd import Config, Reconstructor, capi  # noqa: E402

D, H, NB, M = 1024, 1000, 64, 7


def event_median(st, fn, calls, reps, warmup=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    count = D * H
    emitted, after = capi.manualavg_plan(M, capi.MANUALAVG_REFERENCE, 0, NB)
    assert (emitted, after) == (8, 0)
    cl = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"))
    cl.copy_f4.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    st = torch.cuda.Stream()
    rec = Reconstructor(Config(width=256, height=8, numfftpoints=256, numdisplaypoints=128))
    rec.set_stream(st.cuda_stream)
    x = torch.from_numpy(np.random.default_rng(4).uniform(1e-5, 50.0, (NB, count)).astype(np.float32)).cuda()
    mean, db = torch.empty((emitted, count), dtype=torch.float32, device="cuda"), torch.empty((emitted, count), dtype=torch.float32, device="cuda")
    nbytes = NB * count * 4 + 2 * emitted * count * 4 + 16 * count
    half = nbytes // 2 // 16 * 16          # the copy reads and writes: half the bytes each way
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rec.manualavg_begin(M, count)

    def add():
        rec.manualavg_add_device(x.data_ptr(), NB, mean.data_ptr(), db.data_ptr(), emitted)

    def copy():
        cl.copy_f4(dst.data_ptr(), src.data_ptr(), half, 0, 0, st.cuda_stream)

    rows = []
    for _ in range(3):                      # the two alternate, so that a drift of the clock shows in both
        rows.append((event_median(st, add, args.calls, args.reps), event_median(st, copy, args.calls, args.reps)))
    assert rec.manualavg_state()[3] == 0
    add_us, copy_us = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    res = dict(op="fdoct_manualavg_add", images=NB, image="%d x %d" % (D, H), manualaverages=M, mode="reference", emitted=emitted,
               mbytes=round(nbytes / 1e6, 1), add_us=round(add_us, 1), add_gbs=round(nbytes / add_us / 1e3, 1),
               copy_f4_same_bytes_us=round(copy_us, 1), copy_gbs=round(2 * half / copy_us / 1e3, 1),
               fraction_of_copy=round(copy_us / add_us, 3), rounds=[[round(a, 1), round(c, 1)] for a, c in rows],
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    rec.set_stream(None)
    rec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/manualavg_bench.py: us per call = median of %d measurements of %d calls back to back, HIP events\n" % (args.reps, args.calls))
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
