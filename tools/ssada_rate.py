"""Transforms per second of the split-spectrum stage (fdoct_ssada, include/fdoct_ssada.h) on device-resident complex A-scans of the
full transform length, through the public interface only: 64 frames of 1000 A-scans x 2048 points (1 GB of pairs), 4 repeats x 16
groups, 4 bands, the depth range n / 2 (1024 depths kept: 2.1 GB of band pairs).

  the stage as a whole   out_decorr and out_power in device memory, windows 1 x 1 and 5 x 5; the band pairs go through the handle's
                         workspace -- at the default cap of 2 GiB in two passes, and at a cap of 4 GiB in one;
  the split alone        out_bands alone, in device memory: the table and the split kernel, nothing else.

transforms = frames x A-scans x (1 + bands): the forward transform of every A-scan and the inverse of every band.  profiles/
dispersion_rate.txt's figure at n = 2048 (9.56e7 transforms/s, 32 candidates a workgroup) is quoted in every line for comparison.

Beside them, in the same run, the same images by torch: torch.fft.fft over the A-scans, the product with the band table, torch.fft.ifft,
the depth range made contiguous, then angiography.angio_device per (group, band) for its out_decorr and out_power, and the mean over
the bands.

--chunk N sets FDOCT_SSADA_CHUNK (bands a workgroup takes; the library ships all of them) before the library loads: a sweep is one
process per value.  Times are device events on the stream the handle is given, around each call: the median of --reps calls after
--warmup.

    python3 tools/ssada_rate.py [--reps 20] [--warmup 3] [--chunk N] [--no-torch] [--append profiles/ssada_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, N, FRAMES, REPEATS, BANDS = 1000, 2048, 64, 4, 4
GROUPS, DC = FRAMES // REPEATS, N // 2
WINDOWS = ((1, 1), (5, 5))
DISPERSION_TRANSFORMS_PER_S = 95619772.0   # profiles/dispersion_rate.txt, n = 2048


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
    """Device-resident pairs (FRAMES, H, N, 2): fully developed speckle, static on the first half of the depths and new in every
    frame on the second, a few counts of noise."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    fixed = 707.0 * torch.randn((1, H, N, 2), generator=g, device="cuda")
    x = 707.0 * torch.randn((FRAMES, H, N, 2), generator=g, device="cuda")
    x[:, :, :N // 2] = fixed[:, :, :N // 2]
    x += 4.0 * torch.randn((FRAMES, H, N, 2), generator=g, device="cuda")
    return x.contiguous()


def rates(ms):
    med = statistics.median(ms)
    tr = FRAMES * H * (1 + BANDS)
    return dict(ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), launches=len(ms), transforms=tr,
                transforms_per_s=round(tr / (med * 1e-3), 0), dispersion_transforms_per_s_same_n=DISPERSION_TRANSFORMS_PER_S,
                input_GB_per_s=round(FRAMES * H * N * 8 / (med * 1e-3) / 1e9, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 timed launches")
    if args.chunk > 0:
        os.environ["FDOCT_SSADA_CHUNK"] = str(args.chunk)
    import torch
    from fdoct_amd import Config, Reconstructor, angiography, ssada
    chunk = args.chunk if 0 < args.chunk < BANDS else None
    lines = []
    with torch.cuda.stream(torch.cuda.Stream()):
        stream = torch.cuda.current_stream()
        rec = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=128))   # the stage reads nothing of the geometry
        rec.set_stream(stream.cuda_stream)
        x = pairs()
        dec = torch.empty(GROUPS * H * DC, dtype=torch.float32, device="cuda")
        pw = torch.empty(GROUPS * H * DC, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        base = dict(frames=FRAMES, repeats=REPEATS, groups=GROUPS, ascans=H, n=N, bands=BANDS, depths=DC, chunk_forced=chunk)

        # the split alone: out_bands in device memory
        bands = torch.empty(FRAMES * BANDS * H * DC * 2, dtype=torch.float32, device="cuda")
        p = ssada.params(repeats=REPEATS, bands=BANDS, n=N)
        ms = timed(lambda: ssada.ssada_device(rec, x.data_ptr(), FRAMES, H, N, p, None, None, None, bands.data_ptr()), args.reps, args.warmup, stream)
        info = ssada.plan(p, FRAMES, H, N)
        lines.append(dict(what="fdoct_ssada, out_bands alone (the table and the split kernel)", lds_bytes=info["lds_bytes"], written_bytes=bands.numel() * 4,
                          written_GB_per_s=round(bands.numel() * 4 / (statistics.median(ms) * 1e-3) / 1e9, 2), **base, **rates(ms)))
        del bands
        torch.cuda.empty_cache()

        # the stage as a whole
        for cap in (0, 4 << 30):
            for win in WINDOWS:
                p = ssada.params(repeats=REPEATS, bands=BANDS, n=N, win=win, max_workspace_bytes=cap)
                info = ssada.plan(p, FRAMES, H, N)
                ms = timed(lambda: ssada.ssada_device(rec, x.data_ptr(), FRAMES, H, N, p, dec.data_ptr(), None, pw.data_ptr(), None), args.reps, args.warmup, stream)
                lines.append(dict(what="fdoct_ssada, out_decorr and out_power", window=list(win), max_workspace_bytes=cap, passes=info["passes"],
                                  groups_per_pass=info["groups_per_pass"], workspace_bytes=info["workspace_bytes"], **base, **rates(ms)))

        # the same images by torch.fft and angio_device per band
        if not args.no_torch and chunk is None:
            table = torch.from_numpy(ssada.band_table(ssada.params(repeats=REPEATS, bands=BANDS, n=N), N)).cuda()
            xc = torch.view_as_complex(x)
            band = torch.empty((FRAMES, H, DC, 2), dtype=torch.float32, device="cuda")
            bd = torch.empty((BANDS, GROUPS * H * DC), dtype=torch.float32, device="cuda")
            bp = torch.empty((BANDS, GROUPS * H * DC), dtype=torch.float32, device="cuda")
            keep = {}
            for win in WINDOWS:
                pa = angiography.params(repeats=REPEATS, win=win)

                def run():
                    z = torch.fft.fft(xc, dim=-1) * (1.0 / N)
                    for m in range(BANDS):
                        a = torch.fft.ifft(z * table[m], dim=-1, norm="forward")
                        band.copy_(torch.view_as_real(a[..., :DC]))
                        angiography.angio_device(rec, band.data_ptr(), FRAMES, H, DC, pa, None, bd[m].data_ptr(), None, bp[m].data_ptr())
                    keep["decorr"], keep["power"] = bd.mean(0), bp.mean(0)

                ms = timed(run, args.reps, args.warmup, stream)
                line = dict(what="torch.fft forward, table product, inverse, then angio_device per band and the band means", window=list(win), **base, **rates(ms))
                stage = [ln for ln in lines if ln.get("window") == list(win) and ln.get("max_workspace_bytes") == 0][0]
                line["stage_speedup"] = round(line["ms"] / stage["ms"], 2)
                lines.append(line)
        torch.cuda.synchronize()
        rec.close()
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/ssada_rate.py: fdoct_ssada on device-resident pairs, 64 frames of 1000 x 2048, 4 repeats x 16 groups, 4 bands, 1024 depths "
                        "kept; transforms = frames x A-scans x (1 + bands); ms = median of device events over `launches` calls; "
                        "dispersion_transforms_per_s_same_n: profiles/dispersion_rate.txt at n = 2048; torch lines: torch.fft and angio_device per band in "
                        "the same run (stage_speedup = its ms over the stage's at the default cap); lines with chunk_forced: FDOCT_SSADA_CHUNK\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
