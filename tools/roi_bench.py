"""Device time of the B-scan readouts (include/fdoct_roi.h) on C2 output batches: 262 dB B-scans of 1000 A-scans x 1024
depths (1.07 GB), both layouts; fdoct_peakhold / fdoct_roi_mean for a 10 x 10 box, a 200 x 300 box (A-scans x depths) and
the whole image, fdoct_ascan_minmax for one A-scan.  HIP events around `reps` back-to-back calls on one stream; us per call,
and GB/s of the bytes each call must read (the box, or the A-scan's depth rows 4..D-1).  Next to it the C2 process_async
step the readouts follow, timed the same way.

    python3 tools/roi_bench.py [--reps 50] [--out profiles/roi_bench.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdoct_amd import DTYPE_U16, LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED, Config, Reconstructor, synth  # noqa: E402

W, H, N, D, NB = 2048, 1000, 2048, 1024, 262
ACHIEVABLE_GBS = 6290.0  # MI355X_MICROARCH.md: float4 copy, measured


def timed(st, fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_background(synth.make_background(W))
    st = torch.cuda.Stream()
    frames = torch.from_numpy(np.tile(synth.make_frames(0, 2, W, H), (NB // 2, 1, 1)).view(np.int16)).cuda()
    db = torch.empty(NB * H * D, dtype=torch.float32, device="cuda")
    out = torch.empty(2 * NB, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rec.set_stream(st.cuda_stream)
    lines = []

    def report(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for layout, lname in ((LAYOUT_ROWMAJOR, "rowmajor"), (LAYOUT_TRANSPOSED, "transposed")):
        # the chain's own output in this layout: what the readouts read in an acquisition loop
        step = timed(st, lambda: rec.process_device(frames.data_ptr(), DTYPE_U16, NB, 0, None, db.data_ptr(), layout), 20)
        report(op="process_async C2", layout=lname, us=round(step, 2))
        boxes = (("10x10", 495, 500, 10, 10), ("200x300", 400, 300, 200, 300), ("full", 0, 0, H, D))
        for name, x, y, w, h in boxes:
            rec.set_peakhold_roi(x, y, w, h, x)
            us = timed(st, lambda: rec.peakhold_device(1, db.data_ptr(), NB, D, H, layout), args.reps)
            nbytes = NB * (w + 1) * h * 4
            report(op="peakhold", layout=lname, roi=name, us=round(us, 2), gbs=round(nbytes / us / 1e3, 1),
                   of_achievable=round(nbytes / us / 1e3 / ACHIEVABLE_GBS, 3), of_c2_step=round(us / step, 4))
            width = min(w, H - 1 - x)  # the strict guard: ascanat + width < ascans
            us = timed(st, lambda: rec.roi_mean_device(db.data_ptr(), NB, D, H, x, min(y, D - 3), width, out.data_ptr(), layout),
                       args.reps)
            nbytes = NB * 3 * width * 4
            report(op="roi_mean", layout=lname, roi="%dx3" % width, us=round(us, 2), gbs=round(nbytes / us / 1e3, 1),
                   of_c2_step=round(us / step, 4))
        fo = out.data_ptr()
        us = timed(st, lambda: rec.ascan_minmax_device(db.data_ptr(), NB, D, H, 500, fo, fo + 4 * NB, layout), args.reps)
        nbytes = NB * (D - 4) * 4
        report(op="ascan_minmax", layout=lname, us=round(us, 2), gbs=round(nbytes / us / 1e3, 1), of_c2_step=round(us / step, 4))
    rec.set_stream(None)
    rec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/roi_bench.py: C2 output batches (%d dB B-scans of %d A-scans x %d depths), us per call from HIP events\n"
                    % (NB, H, D))
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
