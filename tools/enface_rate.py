"""Time of the en-face stage (fdoct_enface, include/fdoct_enface.h) on a device-resident volume, through the public interface only:
256 positions x 1000 A-scans x 1024 depths of floats (1 GiB), the volume fdoct_angio leaves of 256 positions of bench.py's C2 image.

  fixed slabs: one over the full depth, and four of 64 depths (128 .. 384); mean, max and argmax, and the mean alone.
  surface-following slabs: mode 2 (relative) with smooth 4 and median 5, four slabs of 64 depths from the surface; all four outputs.

read bytes = what the call's kernels read of the volume: per A-scan the blocks of 256 depths that meet one of its slabs (with a
surface: counted from the surface the call returned), and for the surface the search range once (the box sums' re-reads and the
second pass are left to the cache and not counted: a lower bound).

Beside each case, in the same run:
  the same images from torch reductions on the same volume: per slab a slice's mean and max (values and indices); for the surface
  avg_pool1d for the box sums, their maximum, the first crossing by argmax of the comparison, a median over unfolded windows, and a
  gather of the slabs;
  the in-tree float4 copy (tools/ubench/copy_f4.hip) moving the same number of bytes as the stage's call reads and writes.

Times are device events on the stream the handle is given, around each call: the median of --reps calls after --warmup.

    python3 tools/enface_rate.py [--reps 20] [--warmup 3] [--append profiles/enface_rate.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, H, D = 256, 1000, 1024
NAMES = ("mean", "max", "argmax", "surface")
FULL = [(0, D)]
FOUR = [(128, 64), (192, 64), (256, 64), (320, 64)]
FOLLOW = [(0, 64), (64, 64), (128, 64), (192, 64)]
SURFACE = dict(surface="relative", threshold=0.5, smooth=4, median=5)


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


def volume():
    """A device-resident volume (P, H, D): noise in front of a surface that wanders over A-scans and positions, an exponentially
    falling speckle behind it."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    depth = torch.arange(D, device="cuda", dtype=torch.float32)[None, None, :]
    r = torch.arange(H, device="cuda", dtype=torch.float32)[None, :, None]
    p = torch.arange(P, device="cuda", dtype=torch.float32)[:, None, None]
    z = 150.0 + 60.0 * torch.sin(r / 40.0) + 30.0 * torch.cos(p / 10.0)
    v = 0.05 * torch.rand((P, H, D), generator=g, device="cuda")
    v += (depth >= z) * torch.exp(-(depth - z).clamp(min=0.0) / 200.0) * (0.5 + torch.rand((P, H, D), generator=g, device="cuda"))
    return v.contiguous()


def summary(ms, moved):
    med = statistics.median(ms)
    return dict(ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms), moved_bytes=moved,
                moved_GB_per_s=round(moved / (med * 1e-3) / 1e9, 2), ascans_per_s=round(P * H / (med * 1e-3), 0))


def read_bytes(slabs, z=None):
    """What the kernels read of the volume: per A-scan the blocks of 256 depths that meet one of its clipped slabs -- from the
    surface the call returned (z: int32 (P, H) on the device, -1: none) where there is one -- and with a surface the search range once."""
    import torch
    if z is None:
        blocks = set()
        for first, count in slabs:
            blocks |= set(range(first // 256, (min(first + count, D) - 1) // 256 + 1))
        return P * H * 4 * 256 * len(blocks)
    z = z.long()
    n = 0
    for k in range((D + 255) // 256):
        meet = torch.zeros_like(z, dtype=torch.bool)
        for first, count in slabs:
            lo, hi = (z + first).clamp(min=0), (z + first + count).clamp(max=D)
            meet |= (z >= 0) & (hi > lo) & (lo < 256 * (k + 1)) & (hi > 256 * k)
        n += int(meet.sum().item()) * min(256, D - 256 * k)
    return 4 * n + P * H * D * 4


def stage_line(rec, v, what, slabs, surface, want, outs, reps, warmup, stream):
    from fdoct_amd import enface
    p = enface.params(slabs=slabs, **(SURFACE if surface else {}))
    info = enface.plan(p, P, H, D)
    ptr = lambda w: outs[w].data_ptr() if w in want else None   # noqa: E731
    ms = timed(lambda: enface.project_into(rec, v.data_ptr(), None, P, H, D, p, ptr("mean"), ptr("max"), ptr("argmax"), ptr("surface")), reps, warmup, stream)
    z = outs["surface"][:P * H].view(P, H) if surface else None
    moved = read_bytes(slabs, z) + sum(P * H * 4 * (1 if w == "surface" else len(slabs)) for w in want)
    return dict(what="fdoct_enface", case=what, slabs=[list(s) for s in slabs], surface=SURFACE if surface else None, outputs=list(want),
                workgroups_on_256_cus=info["workgroups"], workspace_bytes=info["workspace_bytes"], **summary(ms, moved))


def torch_line(v, what, slabs, surface, want, reps, warmup, stream):
    import torch
    import torch.nn.functional as F
    keep = {}
    span = torch.arange(max(c for _, c in slabs), device="cuda")

    def fixed():
        for s, (first, count) in enumerate(slabs):
            part = v[:, :, first:first + count]
            if "mean" in want:
                keep["mean", s] = part.mean(-1)
            if "max" in want or "argmax" in want:
                keep["max", s], keep["argmax", s] = part.max(-1)

    def follow():
        B = F.avg_pool1d(v.view(P * H, 1, D), SURFACE["smooth"], stride=1)[:, 0] * SURFACE["smooth"]
        hit = B >= SURFACE["threshold"] * B.max(-1, keepdim=True).values
        z0 = hit.to(torch.uint8).argmax(-1).view(P, H)
        half = SURFACE["median"] // 2
        z = F.pad(z0[:, None].float(), (half, half), mode="replicate")[:, 0].unfold(1, SURFACE["median"], 1).median(-1).values.long()
        keep["surface"] = z
        for s, (first, count) in enumerate(slabs):
            idx = (z[:, :, None] + first + span[None, None, :count]).clamp(0, D - 1)
            part = torch.gather(v, 2, idx)
            keep["mean", s] = part.mean(-1)
            keep["max", s], keep["argmax", s] = part.max(-1)

    ms = timed(follow if surface else fixed, reps, warmup, stream)
    return dict(what="torch reductions on the same volume", case=what, outputs=list(want), ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
                max_ms=round(max(ms), 4), launches=len(ms))


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
        v = volume()
        outs = {w: torch.empty(4 * P * H, dtype=torch.int32 if w in ("argmax", "surface") else torch.float32, device="cuda") for w in NAMES}
        torch.cuda.synchronize()
        cases = (("fixed, one slab over the full depth", FULL, False, NAMES[:3]), ("fixed, one slab over the full depth", FULL, False, ("mean",)),
                 ("fixed, four slabs of 64 depths", FOUR, False, NAMES[:3]), ("fixed, four slabs of 64 depths", FOUR, False, ("mean",)),
                 ("surface-following, four slabs of 64 depths", FOLLOW, True, NAMES))
        for what, slabs, surface, want in cases:
            line = stage_line(rec, v, what, slabs, surface, want, outs, args.reps, args.warmup, stream)
            c = copy_line(cl, line["moved_bytes"], args.reps, args.warmup, stream)
            line["copy_f4_same_bytes_ms"] = c["ms"]
            line["fraction_of_copy"] = round(c["ms"] / line["ms"], 3)
            t = torch_line(v, what, slabs, surface, want, args.reps, args.warmup, stream)
            t["stage_speedup"] = round(t["ms"] / line["ms"], 2)
            lines += [line, c, t]
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
        rec.close()
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/enface_rate.py: fdoct_enface on a device-resident volume of 256 positions x 1000 A-scans x 1024 depths; moved_bytes = per A-scan the blocks of "
                        "256 depths that meet a slab (with a surface: from the surface returned, plus the search range once, a lower bound) read + outputs written; ms = median of device "
                        "events over `launches` calls; copy_f4 lines: the in-tree float4 copy moving the same bytes (fraction_of_copy = its ms over the "
                        "stage's); torch lines: the same images from torch reductions in the same run (stage_speedup = its ms over the stage's)\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
