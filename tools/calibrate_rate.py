"""Wall time of BscanDark's calibration (the d / r / t keys and data_yb = (yr - yd) + (ys - yd), BscanDark.cpp:996, 1005-1222) at
C2's frame shape (2048 x 1000 u16, 16 frames per capture, frames device-resident), two ways on one handle in one process, through
the public interface only:

  (a) host recipe   three fdoct_capture_reference(FDOCT_REF_NONE, .., out_host) calls -- each downloads its H x W doubles,
                    normalises them on the host and, with lowpassfilter, uploads and downloads them once more --, the composition
                    on the host (numpy, one vectorised expression: what a compiled loop costs or less), fdoct_set_background
  (b) on the device three fdoct_calibrate_capture calls (dark, reference, sample; no out_host) and fdoct_calibrate_compose
                    (include/fdoct_calibrate.h)

Both end with the same background in the handle (compared bit for bit); (b) also leaves the dark capture as the handle's dark
frame, which (a) would need one more setter call for.  Every figure is the median of `--reps` synchronous runs after a warm-up.

    python3 tools/calibrate_rate.py [--lowpass 0|1] [--normalize 0|1] [--reps 10] [--append profiles/calibrate_rate.txt]

--normalize 0: donotnormalize = 1, rowwisenormalize = 0 (the sums are divided by the frame count); --normalize 1: both
normalisations run (rowwisenormalize = 1, donotnormalize = 0).  One invocation measures one setting and appends its lines to
--append, so that a driver can run each setting as a step of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdoct_amd import (CAL_DARK, CAL_REFERENCE, CAL_SAMPLE, DTYPE_U16, REF_BACKGROUND, REF_NONE, Config,  # noqa: E402
                       Reconstructor)

W, H, N, D = 2048, 1000, 2048, 1024
NFRAMES = 16


def make_frames(seed, level):
    """NFRAMES device-resident camera frames around `level` counts."""
    rng = np.random.default_rng(seed)
    f = rng.integers(level // 2, level, (NFRAMES, H, W), dtype=np.uint16)
    t = torch.from_numpy(f.view(np.int16)).cuda()
    torch.cuda.synchronize()
    return t


def wall_median(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lowpass", type=int, default=0)
    ap.add_argument("--normalize", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    flags = dict(rowwisenormalize=1, donotnormalize=0) if args.normalize else dict(rowwisenormalize=0, donotnormalize=1)
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, **flags))
    rec.set_capture_options(lowpass=bool(args.lowpass))
    dark, ref, smp = make_frames(1, 4000), make_frames(2, 40000), make_frames(3, 60000)

    def host_recipe():
        yd = rec.capture_reference_device(REF_NONE, dark.data_ptr(), DTYPE_U16, NFRAMES, 0, out=True)
        yr = rec.capture_reference_device(REF_NONE, ref.data_ptr(), DTYPE_U16, NFRAMES, 0, out=True)
        ys = rec.capture_reference_device(REF_NONE, smp.data_ptr(), DTYPE_U16, NFRAMES, 0, out=True)
        rec.set_background((yr - yd) + (ys - yd))

    def on_device():
        rec.calibrate_capture_device(CAL_DARK, dark.data_ptr(), DTYPE_U16, NFRAMES, 0)
        rec.calibrate_capture_device(CAL_REFERENCE, ref.data_ptr(), DTYPE_U16, NFRAMES, 0)
        rec.calibrate_capture_device(CAL_SAMPLE, smp.data_ptr(), DTYPE_U16, NFRAMES, 0)
        rec.calibrate_compose()

    a_ms = wall_median(host_recipe, args.reps)
    yb_a = rec.get_reference(REF_BACKGROUND)
    b_ms = wall_median(on_device, args.reps)
    yb_b = rec.get_reference(REF_BACKGROUND)
    same = bool(yb_a.shape == yb_b.shape and np.array_equal(yb_a.view(np.uint64), yb_b.view(np.uint64)))
    rec.close()
    setting = dict(lowpassfilter=int(bool(args.lowpass)), rowwisenormalize=flags["rowwisenormalize"], donotnormalize=flags["donotnormalize"])
    lines = [
        dict(way="(a) host recipe: 3 x fdoct_capture_reference(NONE, out_host), host composition, fdoct_set_background", **setting,
             ms=round(a_ms[0], 2), min_ms=round(a_ms[1], 2), max_ms=round(a_ms[2], 2)),
        dict(way="(b) on the device: 3 x fdoct_calibrate_capture, fdoct_calibrate_compose", **setting,
             ms=round(b_ms[0], 2), min_ms=round(b_ms[1], 2), max_ms=round(b_ms[2], 2),
             a_over_b=round(a_ms[0] / b_ms[0], 2), same_background_bits=same),
    ]
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/calibrate_rate.py: BscanDark's calibration at C2's frame shape (%d x %d u16, %d frames per capture, "
                        "frames in HBM); ms = median wall time of %d synchronous runs\n" % (W, H, NFRAMES, args.reps))
            for kw in lines:
                f.write(json.dumps(kw) + "\n")
    if not same:
        sys.exit("the two ways left different backgrounds")


if __name__ == "__main__":
    main()
