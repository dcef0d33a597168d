"""Pixels per second of the coherent-averaging stage (fdoct_cxavg, include/fdoct_cxavg.h) on device-resident complex A-scans,
through the public interface only, on bench.py's C2 image (1000 A-scans x 1024 depths), 64 frames (500 MiB of pairs):

  4 repeats x 16 groups, and 2 repeats x 32 groups; align 0, 1 and 2; all four outputs, and out_mag alone;
  the sliding average: 4 repeats, stride 1 (61 groups, every frame read by up to four of them), align 1.

pixels = groups x ascans x depths of output; input GB/s = the 64 frames' bytes once over the call's time, whatever the stride.

Beside each shape, in the same run:
  the composition a user writes without the stage: torch on the same device-resident pairs viewed as complex -- the correlation
  with the ref and its sum over the range, the phasor, the turned sum over the repeats, the moduli and their sum, the four images;
  the in-tree float4 copy (tools/ubench/copy_f4.hip) moving the same number of bytes as the stage's call reads once and writes.

--library times another build of libfdoct_cxavg.so (say one whose kCxaRegPairs is 0, so that the headline shape takes the
streaming form) in place of the package's: the lines carry its name.

Times are device events on the stream the handle is given, around each call: the median of --reps calls after --warmup.

    python3 tools/cxavg_rate.py [--reps 20] [--warmup 3] [--library PATH] [--append profiles/cxavg_rate.txt]
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
SHAPES = ((4, 4, 16), (2, 2, 32))          # repeats, stride, groups
SLIDING = (4, 1, 61)
NAMES = ("mean", "mag", "incoh", "coh")
BYTES = {"mean": 8, "mag": 4, "incoh": 4, "coh": 4}


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
    frame on the second, a few counts of noise, and a phase per (frame, A-scan) that every depth shares."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    fixed = 707.0 * torch.randn((1, H, D, 2), generator=g, device="cuda")
    x = 707.0 * torch.randn((FRAMES, H, D, 2), generator=g, device="cuda")
    x[:, :, :D // 2] = fixed[:, :, :D // 2]
    x += 4.0 * torch.randn((FRAMES, H, D, 2), generator=g, device="cuda")
    phase = 6.2831853 * torch.rand((FRAMES, H, 1), generator=g, device="cuda")
    xc = torch.view_as_complex(x.contiguous()) * torch.polar(torch.ones_like(phase), phase)
    return torch.view_as_real(xc).contiguous()


def rates(groups, ms, moved):
    med = statistics.median(ms)
    px = groups * H * D
    return dict(ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms), pixels=px,
                pixels_per_s=round(px / (med * 1e-3), 0), input_GB_per_s=round(FRAMES * H * D * 8 / (med * 1e-3) / 1e9, 2),
                moved_GB_per_s=round(moved / (med * 1e-3) / 1e9, 2))


def stage_line(rec, x, shape, align, want, outs, reps, warmup, stream, library):
    from fdoct_amd import coherent
    repeats, stride, groups = shape
    p = coherent.params(repeats=repeats, stride=stride, ref=0, align=align)
    info = coherent.plan(p, FRAMES, H, D)
    assert info["groups"] == groups
    ptr = lambda w: outs[w].data_ptr() if w in want else None   # noqa: E731
    ms = timed(lambda: coherent.cxavg_device(rec, x.data_ptr(), FRAMES, H, D, p, ptr("mean"), ptr("mag"), ptr("incoh"), ptr("coh")), reps, warmup, stream)
    moved = FRAMES * H * D * 8 + sum(BYTES[w] for w in want) * groups * H * D
    line = dict(what="fdoct_cxavg", repeats=repeats, stride=stride, groups=groups, ascans=H, depths=D, align=align, outputs=list(want),
                form=info["form"], workspace_bytes=info["workspace_bytes"], moved_bytes=moved, **rates(groups, ms, moved))
    if library:
        line["library"], line["form"] = os.path.basename(library), None    # plan is the package's: the other build decides for itself
    return line


def composition_line(x, shape, align, reps, warmup, stream):
    import torch
    repeats, stride, groups = shape
    assert stride == repeats
    xg = torch.view_as_complex(x).view(groups, repeats, H, D)
    keep = {}

    def run():
        if align:
            C = (xg * xg[:, :1].conj()).sum(-1 if align == 1 else (-2, -1))
            m = C.abs()
            U = torch.where(m > 0, C.conj() / m, torch.ones_like(C))
            S = (xg * (U[..., None] if align == 1 else U[..., None, None])).sum(1)
        else:
            S = xg.sum(1)
        A = xg.abs().sum(1)
        keep["mean"] = S / repeats
        keep["mag"] = keep["mean"].abs()
        keep["incoh"] = A / repeats
        keep["coh"] = torch.where(A > 0, S.abs() / A, torch.zeros_like(A))

    ms = timed(run, reps, warmup, stream)
    moved = FRAMES * H * D * 8 + sum(BYTES.values()) * groups * H * D
    return dict(what="torch on the complex view (correlation, phasor, turned sum, moduli, four images)", repeats=repeats, stride=stride, groups=groups,
                ascans=H, depths=D, align=align, **rates(groups, ms, moved))


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
    ap.add_argument("--library", default=None)
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
        if args.library:
            other = ctypes.CDLL(os.path.abspath(args.library))
            other.fdoct_cxavg.argtypes = rec.lib.fdoct_cxavg.argtypes
            rec.lib.fdoct_cxavg = other.fdoct_cxavg
        rec.set_stream(stream.cuda_stream)
        x = pairs()
        torch.cuda.synchronize()
        for shape in SHAPES + (SLIDING,):
            groups = shape[2]
            outs = {w: torch.empty(groups * H * D * BYTES[w] // 4, dtype=torch.float32, device="cuda") for w in NAMES}
            for align in ((0, 1, 2) if shape != SLIDING else (1,)):
                full = stage_line(rec, x, shape, align, NAMES, outs, args.reps, args.warmup, stream, args.library)
                one = stage_line(rec, x, shape, align, ("mag",), outs, args.reps, args.warmup, stream, args.library)
                for line in (full, one):
                    c = copy_line(cl, line["moved_bytes"], args.reps, args.warmup, stream)
                    line["copy_f4_same_bytes_ms"] = c["ms"]
                    line["fraction_of_copy"] = round(c["ms"] / line["ms"], 3)
                    lines += [line, c]
                if shape != SLIDING and not args.library:
                    comp = composition_line(x, shape, align, args.reps, args.warmup, stream)
                    comp["stage_speedup"] = round(comp["ms"] / full["ms"], 2)
                    lines.append(comp)
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
                f.write("# tools/cxavg_rate.py: fdoct_cxavg on device-resident pairs, 64 frames of 1000 x 1024; pixels = groups x ascans x depths; "
                        "input_GB_per_s = the 64 frames' bytes once over ms, moved_GB_per_s = frames read once + outputs written over ms; ms = median of device "
                        "events over `launches` calls; form 1 = register, 2 = streaming; copy_f4 lines: the in-tree float4 copy moving the same bytes "
                        "(fraction_of_copy = its ms over the stage's); composition lines: torch on the complex view in the same run (stage_speedup = its ms "
                        "over the stage's with all four outputs); lines with `library` time another build of the add-on library\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
