"""Pixel-pairs per second of the angiography stage (fdoct_angio, include/fdoct_angio.h) on device-resident complex A-scans, through
the public interface only, on bench.py's C2 image (1000 A-scans x 1024 depths), 64 frames (500 MiB of pairs):

  4 repeats x 16 groups, and 2 repeats x 32 groups; window 1 x 1 and 5 x 5; all four outputs, and out_cdecorr alone; no bulk
  correction, and for the 4 x 16 shape out_cdecorr alone with a bulk range of 256 depths as well.

pixel-pairs = groups x (repeats - 1) x ascans x depths; input GB/s = the pairs' bytes once over the call's time.

Beside each shape and window, in the same run:
  the composition a user writes without the stage: per group doppler_device (frames, lag 1, the same window; out_corr and
  out_power), then torch: the sums over the pairs and their ratio for the complex decorrelation, |X|^2 per frame and its variance
  over the repeats, the amplitude products and half sums, each through avg_pool2d where the window is not 1 x 1, for the other two;
  the in-tree float4 copy (tools/ubench/copy_f4.hip) moving the same number of bytes as the stage's call reads and writes.

Times are device events on the stream the handle is given, around each call: the median of --reps calls after --warmup.

    python3 tools/angio_rate.py [--reps 20] [--warmup 3] [--append profiles/angio_rate.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, D, FRAMES = 1000, 1024, 64
SHAPES = ((4, 16), (2, 32))          # repeats, groups
WINDOWS = ((1, 1), (5, 5))
NAMES = ("var", "decorr", "cdecorr", "power")


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


def pairs():
    """Device-resident pairs (FRAMES, H, D, 2): fully developed speckle, static on the first half of the depths and new in every
    frame on the second, a few counts of noise."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    fixed = 707.0 * torch.randn((1, H, D, 2), generator=g, device="cuda")
    x = 707.0 * torch.randn((FRAMES, H, D, 2), generator=g, device="cuda")
    x[:, :, :D // 2] = fixed[:, :, :D // 2]
    x += 4.0 * torch.randn((FRAMES, H, D, 2), generator=g, device="cuda")
    return x.contiguous()


def rates(repeats, groups, ms, moved):
    med = statistics.median(ms)
    pp = groups * (repeats - 1) * H * D
    return dict(ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms), pixel_pairs=pp,
                pixel_pairs_per_s=round(pp / (med * 1e-3), 0), input_GB_per_s=round(FRAMES * H * D * 8 / (med * 1e-3) / 1e9, 2),
                moved_GB_per_s=round(moved / (med * 1e-3) / 1e9, 2))


def stage_line(rec, x, repeats, groups, win, want, bulk, outs, reps, warmup, stream):
    from fdoct_amd import angiography
    p = angiography.params(repeats=repeats, win=win, bulk=bulk)
    info = angiography.plan(p, FRAMES, H, D)
    ptr = lambda w: outs[w].data_ptr() if w in want else None   # noqa: E731
    ms = timed(lambda: angiography.angio_device(rec, x.data_ptr(), FRAMES, H, D, p, ptr("var"), ptr("decorr"), ptr("cdecorr"), ptr("power")),
               reps, warmup, stream)
    moved = FRAMES * H * D * 8 + len(want) * groups * H * D * 4
    return dict(what="fdoct_angio", repeats=repeats, groups=groups, ascans=H, depths=D, window=list(win), outputs=list(want), bulk=list(bulk) if bulk else None,
                tiles=info["tiles"], workspace_bytes=info["workspace_bytes"], moved_bytes=moved, **rates(repeats, groups, ms, moved))


def composition_line(rec, x, repeats, groups, win, reps, warmup, stream):
    import torch
    import torch.nn.functional as F
    from fdoct_amd import capi
    corr = torch.empty((repeats - 1, H, D, 2), dtype=torch.float32, device="cuda")
    power = torch.empty((repeats - 1, H, D), dtype=torch.float32, device="cuda")
    pad = ((win[0] - 1) // 2, (win[1] - 1) // 2)
    keep = {}
    # the terms in each pixel's truncated window
    cnt = F.avg_pool2d(torch.ones((1, 1, H, D), device="cuda"), win, stride=1, padding=pad, count_include_pad=True)[0, 0] * (win[0] * win[1])

    def box(a):   # the mean over the window (a: (n, H, D)); odd windows only
        return a if win == (1, 1) else F.avg_pool2d(a[:, None], win, stride=1, padding=pad, count_include_pad=False)[:, 0]

    def run():
        for g in range(groups):
            xg = x[g * repeats:(g + 1) * repeats]
            rec.doppler_device(xg.data_ptr(), repeats, H, D, capi.DOPPLER_FRAMES, 1, None, corr.data_ptr(), power.data_ptr(), win=win)
            s = corr.sum(0)
            keep["cdecorr"] = 1.0 - torch.hypot(s[..., 0], s[..., 1]) / (power.sum(0) * cnt)
            inten = xg[..., 0].square() + xg[..., 1].square()
            keep["var"] = box(inten.var(0, unbiased=False)[None])[0]
            keep["power"] = box(inten.mean(0)[None])[0]
            amp = inten.sqrt()
            keep["decorr"] = 1.0 - (box(amp[:-1] * amp[1:]) / box(0.5 * (inten[:-1] + inten[1:]))).mean(0)

    ms = timed(run, reps, warmup, stream)
    moved = FRAMES * H * D * 8 + 4 * groups * H * D * 4
    return dict(what="doppler_device per group + torch (sums over pairs, variance, amplitude products, avg_pool2d)", repeats=repeats, groups=groups, ascans=H,
                depths=D, window=list(win), **rates(repeats, groups, ms, moved))


def copy_line(cl, moved, reps, warmup, stream):
    import torch
    half = (moved // 2) // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    src.zero_()

    def run():
        assert cl.copy_f4(dst.data_ptr(), src.data_ptr(), half, 0, 0, stream.cuda_stream) == 0

    ms = timed(run, reps, warmup, stream)
    med = statistics.median(ms)
    return dict(what="copy_f4 of the same bytes", moved_bytes=2 * half, ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms),
                moved_GB_per_s=round(2 * half / (med * 1e-3) / 1e9, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 timed launches")
    import torch
    from fdoct_amd import Config, Reconstructor
    cl = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"))
    cl.copy_f4.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lines = []
    with torch.cuda.stream(torch.cuda.Stream()):
        stream = torch.cuda.current_stream()
        rec = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage reads nothing of the geometry
        rec.set_stream(stream.cuda_stream)
        x = pairs()
        torch.cuda.synchronize()
        for repeats, groups in SHAPES:
            outs = {w: torch.empty(groups * H * D, dtype=torch.float32, device="cuda") for w in NAMES}
            for win in WINDOWS:
                full = stage_line(rec, x, repeats, groups, win, NAMES, None, outs, args.reps, args.warmup, stream)
                one = stage_line(rec, x, repeats, groups, win, ("cdecorr",), None, outs, args.reps, args.warmup, stream)
                comp = composition_line(rec, x, repeats, groups, win, args.reps, args.warmup, stream)
                comp["stage_speedup"] = round(comp["ms"] / full["ms"], 2)
                for line in (full, one):
                    c = copy_line(cl, line["moved_bytes"], args.reps, args.warmup, stream)
                    line["copy_f4_same_bytes_ms"] = c["ms"]
                    line["fraction_of_copy"] = round(c["ms"] / line["ms"], 3)
                    lines += [line, c]
                lines.append(comp)
            if repeats == 4:
                lines.append(stage_line(rec, x, repeats, groups, (5, 5), ("cdecorr",), (100, 256), outs, args.reps, args.warmup, stream))
            del outs
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
        rec.close()
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/angio_rate.py: fdoct_angio on device-resident pairs, 64 frames of 1000 x 1024; pixel_pairs = groups x (repeats - 1) x ascans x "
                        "depths; input_GB_per_s = the pairs' bytes once over ms, moved_GB_per_s = pairs read + outputs written over ms; ms = median of device "
                        "events over `launches` calls; copy_f4 lines: the in-tree float4 copy moving the same bytes (fraction_of_copy = its ms over the "
                        "stage's); composition lines: doppler_device per group + torch in the same run (stage_speedup = its ms over the stage's with all "
                        "four outputs)\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
