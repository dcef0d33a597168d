"""Device time of BscanDark's low-pass filter (include/fdoct_lowpass.h) through the public interface only:

  * lowpass_rows_kernel alone on device-resident doubles, 2048 x 1000 and 1280 x 960: the tool starts itself once more under
    `rocprofv3 --kernel-trace --stats`; that child calls fdoct_lowpass_rows (device memory on both sides) repeatedly and the
    kernel's durations are read from its trace.  Next to each: the f64 fmas the kernel issues for its sums (analysis 2 W f,
    synthesis 2 (W / 2) f for the conjugate pairs -- the recurrences that advance the phasors come on top and are not counted)
    per second against the card's vector f64 peak, and the bytes it must move (the rows in, the rows out);
  * the same launches between HIP events on the handle's stream;
  * the whole fdoct_capture_reference(DARK) call on 16 device-resident 2048 x 1000 u16 frames (wall clock: it is synchronous)
    with the low-pass option off and on, the difference, and its three parts measured on their own: 16 MB of pageable doubles
    to the device, the kernel, 16 MB back;
  * the same result by hand, which is what a host does without the option: the capture with the option off, lpfilter in numpy
    (tests/lowpass_model.py::lpfilter_truth) on the host, fdoct_set_dark.  The two results are compared under the parity rule.

Every figure is the median of `--reps` measurements after a warm-up.

    python3 tools/lowpass_bench.py [--reps 15] [--out profiles/lowpass_bench.txt]
"""
import argparse
import csv
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

from fdoct_amd import DTYPE_U16, REF_DARK, Config, Reconstructor  # noqa: E402

W, H, N, D = 2048, 1000, 2048, 1024
SHAPES = [(1000, 2048), (960, 1280)]                # (rows, width) of the kernel legs, in the order the child runs them
TRACE_WARMUP = 2
F64_PEAK_FMAS = 78.6e12 / 2                         # vector f64: half the 157.3 TFLOPS vector f32 rate (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz)


def fmas(rows, width):
    f = width // 10
    return rows * (2 * width * f + 2 * (width // 2) * max(f - 1, 0))


def device_rows(rows, width):
    x = torch.from_numpy(np.random.default_rng(2).uniform(0.0001, 1.0, (rows, width))).cuda()
    torch.cuda.synchronize()
    return x


def trace_leg(reps):
    """The child under rocprofv3: every shape's filter TRACE_WARMUP + reps times, in SHAPES' order."""
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    for rows, width in SHAPES:
        x, y = device_rows(rows, width), torch.empty(rows, width, dtype=torch.float64, device="cuda")
        for _ in range(TRACE_WARMUP + reps):
            rec.lowpass_rows_device(x.data_ptr(), rows, width, 0, y.data_ptr())
        rec.synchronize()
    rec.close()
    print(json.dumps({"legs": len(SHAPES)}), flush=True)


def kernel_legs_from_trace(reps):
    tmp = tempfile.mkdtemp(prefix="lowpass_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "lowpass", "--",
               sys.executable, os.path.abspath(__file__), "--trace-leg", "--reps", str(reps)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        trace = glob.glob(os.path.join(tmp, "**", "lowpass_kernel_trace.csv"), recursive=True)[0]
        rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
        durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "lowpass_rows_kernel" in r["Kernel_Name"]]
        per = TRACE_WARMUP + reps
        assert len(durs) == per * len(SHAPES), len(durs)
        return {s: statistics.median(durs[i * per + TRACE_WARMUP:(i + 1) * per]) for i, s in enumerate(SHAPES)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def event_median(st, fn, reps, inner=4, warmup=3):
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
        torch.cuda.synchronize()
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
    legs = kernel_legs_from_trace(args.reps)

    def kernel_line(how, rows, width, us):
        n = fmas(rows, width)
        report(op="lowpass_rows_kernel", how=how, rows=rows, width=width, us=round(us, 2), f64_gfma_per_s=round(n / us / 1e3, 1),
               of_f64_peak=round(n / us * 1e6 / F64_PEAK_FMAS, 3), mbytes_moved=round(2 * rows * width * 8 / 1e6, 2),
               gbs=round(2 * rows * width * 8 / us / 1e3, 1))

    for (rows, width), us in legs.items():
        kernel_line("kernel trace", rows, width, us)

    import lowpass_model
    st = torch.cuda.Stream()
    rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D))
    rec.set_stream(st.cuda_stream)
    for rows, width in SHAPES:
        x, y = device_rows(rows, width), torch.empty(rows, width, dtype=torch.float64, device="cuda")
        us = event_median(st, lambda: rec.lowpass_rows_device(x.data_ptr(), rows, width, 0, y.data_ptr()), args.reps)
        kernel_line("HIP events", rows, width, us)
    rec.set_stream(None)

    # the capture: option off (the library before the option existed), option on, and the parts of the difference
    n = 16
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 65536, (n, H, W), dtype=np.uint16).view(np.int16)).cuda()
    torch.cuda.synchronize()
    capture = lambda: rec.capture_reference_device(REF_DARK, frames.data_ptr(), DTYPE_U16, n, 0)   # noqa: E731
    off_us = wall_median(capture, args.reps)
    plain = rec.get_reference(REF_DARK)
    rec.set_capture_options(lowpass=True)
    on_us = wall_median(capture, args.reps)
    filtered = rec.get_reference(REF_DARK)
    rec.set_capture_options()
    report(op="fdoct_capture_reference(DARK), 16 device frames, lowpass off, whole call", us=round(off_us, 1))
    report(op="fdoct_capture_reference(DARK), 16 device frames, lowpass on, whole call", us=round(on_us, 1), extra_us=round(on_us - off_us, 1))
    host = np.ascontiguousarray(plain)
    dev = torch.empty(H, W, dtype=torch.float64, device="cuda")
    up_us = wall_median(lambda: dev.copy_(torch.from_numpy(host)), args.reps)
    down_us = wall_median(lambda: dev.cpu(), args.reps)
    report(op="parts of the extra time: 16 MB of pageable doubles to the device / lowpass_rows_kernel / 16 MB back", upload_us=round(up_us, 1),
           kernel_us=round(legs[(H, W)], 1), download_us=round(down_us, 1))
    whole_us = wall_median(lambda: rec.lowpass_rows(host), args.reps)
    report(op="fdoct_lowpass_rows, 2048 x 1000, host memory on both sides (upload, kernel, download, a fresh result array)", us=round(whole_us, 1))

    def by_hand():
        rec.capture_reference_device(REF_DARK, frames.data_ptr(), DTYPE_U16, n, 0)
        rec.set_dark(lowpass_model.lpfilter_truth(rec.get_reference(REF_DARK)))
    hand_us = wall_median(by_hand, max(3, args.reps // 3))
    by_hand_result = rec.get_reference(REF_DARK)
    worst, excess = lowpass_model.parity(filtered, plain, by_hand_result)
    report(op="by hand: the capture with the option off, lpfilter in numpy float64 on the host, fdoct_set_dark", us=round(hand_us, 1),
           ratio_by_hand_over_library=round(hand_us / on_us, 2), library_vs_by_hand_err_over_tol=float("%.3e" % worst),
           within_parity_rule=bool(excess <= 0))
    rec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/lowpass_bench.py: doubles, device-resident unless said otherwise; us = median of %d measurements\n" % args.reps)
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
