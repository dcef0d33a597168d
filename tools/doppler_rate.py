"""GB/s of the Doppler stage (fdoct_doppler, include/fdoct_doppler.h) for the bytes it must move, on device-resident complex
A-scans of C2's pair shape (1000 A-scans x 1024 depths a frame), through the public interface only:

  windows 1 x 1 and 4 x 8, both axes (lag 1), with and without the bulk correction; out_phase alone is asked for (the use the
  stage is for), and once all three outputs.  The bytes that must move are the input once (8 B a pair -- with the lag partner a
  pair is read twice, which a cache may or may not absorb: the figure does not count it) and the outputs once.
  Next to them the in-tree 16-bytes-per-lane copy (tools/ubench/copy_f4.hip, what bench.py --full quotes) on as many bytes, where
  tools/ubench/libcopy_f4.so has been built, and torch's device-to-device copy.

  Then, on C2's handle (2048 -> 2048, D 1024, 1000 rows, u16 frames in device memory): process_doppler_device plus the download of
  the phase image, against process_complex_device plus the download of the complex A-scans (what INTEGRATION 2i's numpy lines
  start from; numpy's own time is not counted), pinned host memory on both.

Times are device events on the stream the handle is given, around each call: the median of --reps launches after --warmup, the ways
alternating so that drift hits them alike.  --frames sets the batch: 64 frames are 0.5 GB of pairs, beyond the Infinity Cache.

    python3 tools/doppler_rate.py [--reps 30] [--warmup 5] [--frames 64] [--append profiles/doppler_rate.txt]
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

from fdoct_amd import Config, Reconstructor, capi, synth  # noqa: E402

H, D = 1000, 1024


def timed(ways, reps, warmup, stream):
    """{name: [ms]}: every way once per round, each between its own pair of events."""
    times = {k: [] for k in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(warmup + reps):
        for k, fn in ways.items():
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if it >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return times


def line(what, ms_list, nbytes, **more):
    ms = statistics.median(ms_list)
    return dict(what=what, ms=round(ms, 4), min_ms=round(min(ms_list), 4), max_ms=round(max(ms_list), 4), launches=len(ms_list),
                bytes=nbytes, gb_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), **more)


def stage(nframes, reps, warmup):
    stream = torch.cuda.current_stream()
    rec = Reconstructor(Config(width=64, height=4, numfftpoints=128, numdisplaypoints=32))   # the stage reads nothing of the geometry
    rec.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(0)
    one = (rng.normal(0, 1e3, (4, H, D)) + 1j * rng.normal(0, 1e3, (4, H, D))).astype(np.complex64)
    d_x = torch.from_numpy(one.view(np.float32).reshape(4, -1)).cuda().repeat((nframes + 3) // 4, 1)[:nframes].contiguous()
    in_bytes = nframes * H * D * 8
    bins = nframes * H * D
    d_ph = torch.empty(bins, dtype=torch.float32, device="cuda")
    d_co = torch.empty(2 * bins, dtype=torch.float32, device="cuda")
    d_pw = torch.empty(bins, dtype=torch.float32, device="cuda")
    ways, nbytes = {}, {}
    for axis, aname in ((capi.DOPPLER_ASCANS, "A-scans"), (capi.DOPPLER_FRAMES, "frames")):
        pi, pr = capi.doppler_size(axis, 1, nframes, H, D)
        for win in ((1, 1), (4, 8)):
            for bulk in (None, True):
                k = "%s, %d x %d%s, phase" % (aname, win[0], win[1], ", bulk" if bulk else "")
                ways[k] = (lambda axis=axis, win=win, bulk=bulk: rec.doppler_device(d_x.data_ptr(), nframes, H, D, axis, 1, d_ph.data_ptr(), None, None,
                                                                                     win=win, bulk=bulk))
                nbytes[k] = in_bytes + pi * pr * D * 4
        k = "%s, 4 x 8, phase + corr + power" % aname
        ways[k] = (lambda axis=axis: rec.doppler_device(d_x.data_ptr(), nframes, H, D, axis, 1, d_ph.data_ptr(), d_co.data_ptr(), d_pw.data_ptr(), win=(4, 8)))
        nbytes[k] = in_bytes + pi * pr * D * 16
    # the copies: as many bytes as the phase-only A-scan call moves, half read and half written
    half = (nbytes["A-scans, 1 x 1, phase"] // 2) // 16 * 16
    src = d_x.view(-1)[:half // 4]
    dst = torch.empty(half // 4, dtype=torch.float32, device="cuda")
    ways["torch device-to-device copy"] = lambda: dst.copy_(src)
    nbytes["torch device-to-device copy"] = 2 * half
    so, note = os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so"), None
    if os.path.exists(so):
        cl = ctypes.CDLL(so)
        cl.copy_f4.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        for vname, variant in (("plain", 0), ("nontemporal", 1)):
            k = "in-tree float4 copy, " + vname
            ways[k] = (lambda variant=variant: cl.copy_f4(dst.data_ptr(), src.data_ptr(), half, variant, 0, stream.cuda_stream))
            nbytes[k] = 2 * half
    else:
        note = "tools/ubench/libcopy_f4.so is not built: no in-tree float4 copy"
    times = timed(ways, reps, warmup, stream)
    rec.close()
    out = [line(k, times[k], nbytes[k], frames=nframes) for k in ways]
    if note:
        out.append(dict(note=note))
    return out


def end_to_end(nframes, reps, warmup):
    stream = torch.cuda.current_stream()
    cfg = Config(width=2048, height=H, numfftpoints=2048, numdisplaypoints=D)
    rec = Reconstructor(cfg)
    rec.set_background(synth.make_background(2048))
    rec.set_stream(stream.cuda_stream)
    base = synth.make_frames(0, 4, 2048, H)
    frames = np.ascontiguousarray(base[np.arange(nframes) % 4])
    d_fr = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
    d_cx = torch.empty(nframes * H * D * 2, dtype=torch.float32, device="cuda")
    d_ph = torch.empty(nframes * (H - 1) * D, dtype=torch.float32, device="cuda")
    h_cx = torch.empty(d_cx.shape, dtype=torch.float32).pin_memory()
    h_ph = torch.empty(d_ph.shape, dtype=torch.float32).pin_memory()

    def with_stage():
        rec.process_doppler_device(d_fr.data_ptr(), capi.DTYPE_U16, nframes, 4096, capi.DOPPLER_ASCANS, 1, d_ph.data_ptr(), None, None, win=(4, 8))
        h_ph.copy_(d_ph, non_blocking=True)

    def with_download():
        rec.process_complex_device(d_fr.data_ptr(), capi.DTYPE_U16, nframes, 4096, d_cx.data_ptr())
        h_cx.copy_(d_cx, non_blocking=True)

    ways = {"process_doppler (A-scans, 4 x 8, phase) + download of the phase": with_stage,
            "process_complex + download of the complex A-scans": with_download}
    times = timed(ways, reps, warmup, stream)
    kernel = rec.last_kernel()
    rec.close()
    out = []
    for k in ways:
        ms = statistics.median(times[k])
        out.append(dict(what=k, frames=nframes, ms=round(ms, 4), min_ms=round(min(times[k]), 4), max_ms=round(max(times[k]), 4), launches=len(times[k]),
                        ascans_per_s=round(nframes * H / (ms * 1e-3), 0), chain_kernel=kernel))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--append", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("at least 20 timed launches")
    with torch.cuda.stream(torch.cuda.Stream()):   # a stream of its own: the handles are given it, and the events bracket their work
        lines = stage(args.frames, args.reps, args.warmup) + end_to_end(min(args.frames, 16), args.reps, args.warmup)
        torch.cuda.synchronize()
    for kw in lines:
        print(json.dumps(kw), flush=True)
    if args.append:
        new = not os.path.exists(args.append)
        with open(args.append, "a") as f:
            if new:
                f.write("# tools/doppler_rate.py: the Doppler stage on device-resident pairs of 1000 x 1024 a frame; bytes = the input once + the "
                        "outputs once; ms = median of device events over `launches` calls, the ways alternating\n")
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
