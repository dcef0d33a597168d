"""Pixel-steps per second of the vibrometry stage (fdoct_vibro, include/fdoct_vibro.h) on device-resident complex A-scans,
through the public interface only, on two shapes:

  M-mode   1 A-scan x 1024 depths, 4096 frames (32 MiB of pairs): few pixels, a long record -- what the chunks are for;
  C2       1000 A-scans x 1024 depths, 64 frames (500 MiB of pairs): bench.py's C2 image over time -- one chunk.

Each with 1 and 8 frequencies, with and without a reference range of 8 depths, all four outputs, the plan's own chunk_steps.
pixel-steps = ascans x depths x (frames - 1); input GB/s = the pairs' bytes once over the call's time (what the call moves on top
-- the frame adjacent chunks share, the partials -- is overhead and is not counted).

Beside each, in the same run, the composition a user writes without the stage: doppler_device (frames, lag 1, a 1 x 1 window, the
phase only), then torch: a cumulative sum over time in double, the mean removed, a lock-in against a (frequencies x frames) table
of phasors, and the rms.  It has no reference correction, so it stands beside the lines without one.

  --sweep: chunk_steps forced to each of a list on both shapes (1 frequency, no reference): what the plan's rule was chosen from.

Times are device events on the stream the handle is given, around each call: the median of --reps calls after --warmup.

    python3 tools/vibro_rate.py [--reps 20] [--warmup 3] [--sweep] [--append profiles/vibro_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"M-mode": (4096, 1, 1024), "C2": (64, 1000, 1024)}   # frames, A-scans, depths
SWEEP = {"M-mode": (4, 8, 16, 32, 64, 128, 256, 512, 1024, 4095), "C2": (8, 16, 32, 63)}
FREQS = (0.11, 0.5, 0.03125, 0.25, 0.3333, 0.07, 0.41, 0.0123)


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


def pairs(T, H, D):
    """Device-resident pairs: speckle of constant amplitude per pixel, a phase that moves by well under pi a frame."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    amp = 900.0 * (0.35 + torch.rand((1, H, D), generator=g, device="cuda"))
    t = torch.arange(T, device="cuda", dtype=torch.float32)[:, None, None]
    phi = 6.2831853 * torch.rand((1, H, D), generator=g, device="cuda") + 1.2 * torch.sin(0.6911504 * t + 6.2831853 * torch.rand((1, H, D), generator=g, device="cuda"))
    x = torch.stack((amp * torch.cos(phi), amp * torch.sin(phi)), -1) + 4.0 * torch.randn((T, H, D, 2), generator=g, device="cuda")
    return x.contiguous()


def rates(T, H, D, ms):
    med = statistics.median(ms)
    steps = H * D * (T - 1)
    return dict(ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms), pixel_steps=steps,
                pixel_steps_per_s=round(steps / (med * 1e-3), 0), input_GB_per_s=round(T * H * D * 8 / (med * 1e-3) / 1e9, 2))


def stage_line(rec, name, x, nfreq, ref, reps, warmup, stream, chunk_steps=0):
    import torch
    from fdoct_amd import vibrometry
    T, H, D = SHAPES[name]
    p = vibrometry.params(freq=FREQS[:nfreq], ref=(100, 8) if ref else None, chunk_steps=chunk_steps)
    info = vibrometry.plan(p, T, H, D)
    amp = torch.empty(nfreq * H * D * 2, dtype=torch.float32, device="cuda")
    rms, drift, power = (torch.empty(H * D, dtype=torch.float32, device="cuda") for _ in range(3))
    ms = timed(lambda: vibrometry.vibro_device(rec, x.data_ptr(), T, H, D, p, amp.data_ptr(), rms.data_ptr(), drift.data_ptr(), power.data_ptr()),
               reps, warmup, stream)
    return dict(what="fdoct_vibro", shape=name, frames=T, ascans=H, depths=D, nfreq=nfreq, reference=bool(ref), chunk_forced=chunk_steps or None,
                chunk_steps=info["chunk_steps"], chunks=info["chunks"], workgroups=info["workgroups"], workspace_bytes=info["workspace_bytes"],
                **rates(T, H, D, ms))


def composition_line(rec, name, x, nfreq, reps, warmup, stream):
    import math
    import torch
    from fdoct_amd import capi
    T, H, D = SHAPES[name]
    phase = torch.empty((T - 1, H, D), dtype=torch.float32, device="cuda")
    t = torch.arange(T, device="cuda", dtype=torch.float64)
    table = torch.stack([torch.exp(-2j * math.pi * nu * t) for nu in FREQS[:nfreq]])          # (nfreq, T) complex128
    zero = torch.zeros((1, H, D), dtype=torch.float64, device="cuda")
    keep = {}

    def run():
        rec.doppler_device(x.data_ptr(), T, H, D, capi.DOPPLER_FRAMES, 1, phase.data_ptr(), None, None)
        phi = torch.cat((zero, torch.cumsum(phase, 0, dtype=torch.float64)), 0)
        res = phi - phi.mean(0, keepdim=True)
        keep["amp"] = (2.0 / T) * torch.einsum("ft,thd->fhd", table, res.to(torch.complex128))
        keep["rms"] = res.square().mean(0).sqrt()
        keep["drift"] = phi[-1]

    ms = timed(run, reps, warmup, stream)
    return dict(what="doppler_device + torch (cumsum, mean, lock-in, rms; no reference, no power)", shape=name, frames=T, ascans=H, depths=D, nfreq=nfreq,
                **rates(T, H, D, ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 timed launches")
    import torch
    from fdoct_amd import Config, Reconstructor
    lines = []
    with torch.cuda.stream(torch.cuda.Stream()):
        stream = torch.cuda.current_stream()
        rec = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage reads nothing of the geometry
        rec.set_stream(stream.cuda_stream)
        for name, (T, H, D) in SHAPES.items():
            x = pairs(T, H, D)
            torch.cuda.synchronize()
            for nfreq in (1, 8):
                stage = [stage_line(rec, name, x, nfreq, ref, args.reps, args.warmup, stream) for ref in (False, True)]
                comp = composition_line(rec, name, x, nfreq, args.reps, args.warmup, stream)
                comp["stage_speedup"] = round(comp["ms"] / stage[0]["ms"], 2)
                lines += stage + [comp]
            if args.sweep:
                for cs in SWEEP[name]:
                    lines.append(stage_line(rec, name, x, 1, False, args.reps, args.warmup, stream, chunk_steps=cs))
            del x
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
        rec.close()
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/vibro_rate.py: fdoct_vibro on device-resident pairs, all four outputs; pixel_steps = ascans x depths x (frames - 1); "
                        "input_GB_per_s = the pairs' bytes once over ms; ms = median of device events over `launches` calls; beside it the composition "
                        "doppler_device + torch in the same run (stage_speedup = its ms over the stage's without a reference); lines with chunk_forced: "
                        "the sweep the plan's rule is from (1 frequency, no reference)\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
