"""A-scans/s of the complex call (fdoct_process_complex, include/fdoct_complex.h) next to fdoct_process_async writing one magnitude
image on the same kernel family, in one process, on device-resident frames, through the public interface only:

  C2's shape            2048 -> 2048, D 1024, 1000 rows, u16.  fdoct_process gives it to the fused kernel; the complex call runs
                        the wave-per-row kernel compiled at run time.  The magnitude image on THAT family is forced by handing
                        the frames over 4 bytes past a 16-byte boundary (the fused kernels read 16-byte vectors and leave such a
                        call to the other families); the fused kernel's own rate on aligned frames is printed for orientation.
  BscanFFT.ini's shape  160 x4 -> 2560, D 320, 120 rows, u8 (the 320 x 240 region of interest after 2 x 2 binning).  The magnitude
                        image runs the library's built-in instantiation of the wave-per-row kernel, the complex call the run-time
                        compiled one with FDOCT_WAVE_OPT_CXOUT.

Both shapes also get the complex call with run-time compilation off (the workgroup-per-row kernel), for orientation.

Per A-scan the complex call writes 8 D bytes where the magnitude image writes 4 D, and skips the square root (and, here, nothing
else: no dB image is asked of either).  Times are the handle's own device events around each call (fdoct_set_timing): the median
of --reps launches after --warmup, the calls alternating between the ways so that drift hits them alike.

    python3 tools/complex_rate.py [--reps 30] [--warmup 5] [--append profiles/complex_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdoct_amd import Config, Reconstructor, capi, synth  # noqa: E402

KERNEL_NAMES = ["none", "fused", "fused, D x H store", "fused, staged", "wave-per-row (built in)", "wave-per-row (run-time compiled)",
                "workgroup-per-row", "long rows"]
# (name, W, M, N, D, H, frame type, frames per call, lambdamin, lambdamax)
SHAPES = [
    ("C2 2048 -> 2048, D 1024, u16", 2048, 1, 2048, 1024, 1000, np.uint16, 64, 816e-9, 884e-9),
    ("BscanFFT.ini 160 x4 -> 2560, D 320, u8", 160, 4, 2560, 320, 120, np.uint8, 512, 840.5e-9, 859.5e-9),
]


def measure(name, W, M, N, D, H, dt, nframes, lmin, lmax, reps, warmup):
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, lambdamin=lmin, lambdamax=lmax)
    rec = Reconstructor(cfg)
    rec.set_background(synth.make_background(W, dtype=dt))
    rec.set_timing(True)
    rec_g = Reconstructor(cfg)   # the same call with run-time compilation off: the workgroup-per-row kernel, for orientation
    rec_g.set_background(synth.make_background(W, dtype=dt))
    rec_g.set_timing(True)
    rec_g.set_jit(False)
    base = synth.make_frames(0, 4, W, H, dtype=dt)
    frames = np.ascontiguousarray(base[np.arange(nframes) % 4])
    es, kdt = frames.itemsize, capi._NP2DT[frames.dtype]
    flat = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    h_bytes = torch.from_numpy(frames.view(np.uint8).reshape(-1))
    flat[:frames.nbytes] = h_bytes.cuda()
    shifted = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    shifted[4:4 + frames.nbytes] = flat[:frames.nbytes]
    rows = nframes * H
    d_mag = torch.empty(rows * D, dtype=torch.float32, device="cuda")
    d_cx = torch.empty(rows * D * 2, dtype=torch.float32, device="cuda")
    d_cx2 = torch.empty(rows * D * 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ways = {
        "complex": lambda: rec.process_complex_device(flat.data_ptr(), kdt, nframes, W * es, d_cx.data_ptr()),
        "magnitude": lambda: rec.process_device(flat.data_ptr(), kdt, nframes, W * es, d_mag.data_ptr(), None),
    }
    if M == 1:   # a fused shape: the magnitude image on the complex call's family
        ways["magnitude, same family"] = lambda: rec.process_device(shifted.data_ptr() + 4, kdt, nframes, W * es, d_mag.data_ptr(), None)
    ways["complex, run-time compilation off"] = lambda: rec_g.process_complex_device(flat.data_ptr(), kdt, nframes, W * es, d_cx2.data_ptr())
    owner = {k: (rec_g if k.endswith("compilation off") else rec) for k in ways}
    times, kernels = {k: [] for k in ways}, {}
    for it in range(warmup + reps):
        for k, fn in ways.items():
            fn()
            t = owner[k].timing()   # (waits for the call's last event)
            kernels[k] = owner[k].last_kernel()
            if it >= warmup:
                times[k].append(t["process_ms"])
    # the two outputs of the last calls agree: |X| against the magnitude image less its epsilon
    X = d_cx.cpu().numpy().view(np.complex64).reshape(rows, D)
    mag = d_mag.cpu().numpy().reshape(rows, D)
    rec.close()
    rec_g.close()
    dev = float(np.max(np.abs(np.abs(X.astype(np.complex128)) + 1e-5 - mag) / (1e-4 * mag + 1e-6 * mag.max(axis=1, keepdims=True))))
    out = []
    for k in ways:
        ms = statistics.median(times[k])
        out.append(dict(shape=name, way=k, kernel=KERNEL_NAMES[kernels[k]], ascans_per_call=rows, ms=round(ms, 4), min_ms=round(min(times[k]), 4),
                        max_ms=round(max(times[k]), 4), launches=len(times[k]), ascans_per_s=round(rows / (ms * 1e-3), 0),
                        bytes_per_ascan=W * es + (8 if k.startswith("complex") else 4) * D))
    ref = "magnitude, same family" if M == 1 else "magnitude"
    cx_ms, ref_ms = statistics.median(times["complex"]), statistics.median(times[ref])
    out.append(dict(shape=name, complex_over_magnitude_same_family=round(ref_ms / cx_ms, 3), modulus_minus_magnitude_over_tolerance=round(dev, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 timed launches")
    lines = []
    for shp in SHAPES:
        lines += measure(*shp, reps=args.reps, warmup=args.warmup)
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/complex_rate.py: the complex call against a magnitude image, device-resident frames; ms = median of the handle's "
                        "device events over `launches` calls, the ways alternating; complex_over_magnitude_same_family = rate of the complex call "
                        "/ rate of the magnitude image on the same kernel family\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
