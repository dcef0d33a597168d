#!/usr/bin/env python3
"""Benchmark of the FD-OCT reconstruction hot path on MI355X.

One "step" = one pass of the fused kernel chain over one batch of synthetic
camera frames that are already resident in HBM.  Workload (BASELINE.json
configs[1], "C2"): 2048-sample x 1000-line u16 frames, N = 2048, D = 1024,
Bartlett-Hann window, 1-row background, whole chain to dB.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line (metric = A-scans/s, whole job).  For N > 1 every
rank owns one GPU and its own frame shard; the only collective is the set-up
broadcast of the constant state (RCCL), so scaling is "weak".

A plain run sets up, ramps the clocks, warms up, times the K steps and prints
the line.  --full adds what else the line can carry (package power, CPU
baselines, the parity check against the oracle, per-stage, half-chip,
division-setting and sustained legs, copy-rate ceilings): untimed extras that
run after the timed region.
"""
import argparse
import glob
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_ACHIEVABLE_GBS = 6290.0  # MI355X_MICROARCH.md: 6.29 TB/s measured (float4 copy, 79 %)
DUMP_BYTES = 60_000_000      # --dump-outputs: at most this many bytes of results

WORKLOADS = {
    # name: (W, H, N, D, A, window, phase)
    "C1": dict(W=1024, H=512, N=1024, D=512, A=1, hann=False, phase=False,
               desc="1024-pt x 512-line u16 frames (configs[0], the reference's own CPU-runnable size)"),
    "C2": dict(W=2048, H=1000, N=2048, D=1024, A=1, hann=False, phase=False,
               desc="2048-pt x 1000-line u16 frames, resample+IDFT+dB chain (BASELINE configs[1])"),
    "C3": dict(W=2048, H=1000, N=2048, D=1024, A=1, hann=True, phase=True,
               desc="C2 + dispersion phase multiply + Hann window (configs[2])"),
    "C4": dict(W=4096, H=2048, N=4096, D=2048, A=16, hann=False, phase=False,
               desc="4096-pt x 2048-line, averaging 16 frames (configs[3])"),
    # configs[4]: the C2 frame, one step = ONE call over a 10 000-frame shard per GPU (41 GB in, 41 GB out); `--gpus 8` gives
    # the stated 8 x 10k batch.  The default workload (C2) runs the same kernel over 262-frame batches.
    "C5": dict(W=2048, H=1000, N=2048, D=1024, A=1, hann=False, phase=False, fps=10000, ring=10000, steps=100,
               desc="2048-pt x 1000-line u16 frames, shards of 10 000 frames per GPU and call (BASELINE configs[4])"),
    # the configuration the reference actually ships (build/BscanFFT.ini:9-12, 25-26, 31-32, 51-52): raw camera frames in,
    # software binning on the GPU (main:958), zero-pad upsampling (main:180-245), non-power-of-two numfftpoints
    "INI": dict(W=160, H=120, N=2560, D=320, A=10, M=4, raw_w=320, raw_h=240, bin=2, bits=8, lmin=840.5e-9, lmax=859.5e-9,
                hann=False, phase=False,
                desc="build/BscanFFT.ini: raw 320 x 240 8-bit frames, 2 x 2 binning, 160 samples x4 zero-pad, numfftpoints 2560, "
                     "320 depth bins, 10 averages (not a BASELINE config; the wave-per-row kernel)"),
    # long rows (BscanFFT.cpp:1146-1147 with a 4096-pixel spectrometer and a x8 zero-pad): 16384 complex points per transform, the
    # most one CU's LDS holds; anything longer runs with the rows in HBM between the steps (fdoct_big.hip)
    "LONG": dict(W=4096, H=64, N=32768, D=2048, A=1, M=8, fps=32, ring=64, steps=20, hann=False, phase=False,
                 desc="4096 samples x8 zero-pad -> numfftpoints 32768, 2048 depth bins, 64 lines per frame (not a BASELINE config; "
                      "the workgroup-per-row kernel with one DFT buffer in place; FDOCT_FORCE_LONG_ROWS=1 puts it on the long-row path: "
                      "rows in HBM, transforms as grouped in-LDS launches)"),
    # the same spectrometer with the shipped x4 multiplier: both DFT buffers of the workgroup-per-row kernel fit the LDS
    "LONG4": dict(W=4096, H=64, N=16384, D=2048, A=1, M=4, fps=64, ring=128, steps=20, hann=False, phase=False,
                  desc="4096 samples x4 zero-pad -> numfftpoints 16384, 2048 depth bins, 64 lines per frame (not a BASELINE config; "
                       "the workgroup-per-row kernel; FDOCT_FORCE_LONG_ROWS=1 puts it on the long-row path)"),
}


def wl_tables(wl):
    """Oracle-side tables / window / phase of a workload (CPU baseline and parity legs only)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as orc
    from fdoct_amd import synth
    W, N, M = wl["W"], wl["N"], wl.get("M", 1)
    idx, frac = orc.tables(W, M, N, wl.get("lmin", synth.LAMBDAMIN), wl.get("lmax", synth.LAMBDAMAX))
    win = synth.hann_window(W) if wl["hann"] else orc.barthann(W)
    phase = synth.dispersion_phase(N) if wl["phase"] else None
    p1 = lambda threads: orc.make_params(W, wl["H"], N, wl["D"], M, threads=threads)  # noqa: E731
    binv = wl.get("bin", 1)

    def prep(chunk):   # the frame-source tail the reference runs on the CPU too: software binning (main:958)
        if binv == 1:
            return chunk
        return np.stack([orc.resize_area(f, binv, binv) for f in chunk])
    return orc, idx, frac, win, phase, p1, prep


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def cpu_baseline_frames_parallel(wl, frames_host, yb, seconds, workers):
    """All-cores CPU figure: `workers` threads, each running the single-threaded restatement on its own frames
    (frames are independent, so this is how a CPU would be used for a batch; the oracle's own intra-frame OpenMP
    stops scaling at its serial passes).  Returns (A-scans/s over all workers, frames processed)."""
    import concurrent.futures
    import threading
    orc, idx, frac, win, phase, p1, prep = wl_tables(wl)
    H, A = wl["H"], wl["A"]
    p = p1(1)
    chunk = np.ascontiguousarray(frames_host[:A])
    orc.process_u16(p, A, 1e-5, prep(chunk), yb, None, win, idx, frac, phase=phase)
    stop = threading.Event()

    def work(_):
        n = 0
        while not stop.is_set():
            orc.process_u16(p, A, 1e-5, prep(chunk), yb, None, win, idx, frac, phase=phase)   # ctypes releases the GIL
            n += A
        return n
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(workers) as ex:
        futs = [ex.submit(work, i) for i in range(workers)]
        time.sleep(seconds)
        stop.set()
        done = sum(f.result() for f in futs)
    dt = time.perf_counter() - t0
    return done * H / dt, done


def cpu_baseline(wl, frames_host, yb, seconds, threads):
    """Times the CPU restatement (oracle, kind 'port') on a bounded sample of the same workload."""
    orc, idx, frac, win, phase, p1, prep = wl_tables(wl)
    H, A = wl["H"], wl["A"]
    p = p1(threads)
    chunk = frames_host[:A]
    orc.process_u16(p, A, 1e-5, prep(chunk), yb, None, win, idx, frac, phase=phase)  # warm-up (page faults, plan)
    rates = []
    t_end = time.perf_counter() + seconds
    nfr = 0
    while time.perf_counter() < t_end or len(rates) < 3:
        t0 = time.perf_counter()
        orc.process_u16(p, A, 1e-5, prep(chunk), yb, None, win, idx, frac, phase=phase)
        dt = time.perf_counter() - t0
        rates.append(A * H / dt)
        nfr += A
        if len(rates) >= 200:
            break
    return float(np.median(rates)), float(np.max(rates)), nfr


class PowerSampler:
    """Package power and shader clock of one GPU while the timed region runs, from the amdgpu hwmon files of its PCI device
    (power1_input in uW, freq1_input in Hz, power1_cap): DESIGN.md 5 argues the fused kernel is bounded by the power cap,
    so the bench line records what the chip drew in THIS run.  Read-only sysfs polling on a helper thread (the launching
    thread spends the region inside synchronize() with the GIL released); everything is None when the files are absent."""

    def __init__(self, device_index, period=0.01):
        self.dir = None
        self.period = period
        self.power, self.freq = [], []
        self._stop = threading.Event()
        self._thread = None
        try:
            bus = self._pci_bus_id(device_index)
            cand = sorted(glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*" % bus))
            if cand and os.path.exists(os.path.join(cand[0], "power1_input")):
                self.dir = cand[0]
        except Exception:
            self.dir = None

    @staticmethod
    def _pci_bus_id(device_index):
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        buf = ctypes.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(device_index)) != 0:
            raise RuntimeError("hipDeviceGetPCIBusId")
        return buf.value.decode().lower()

    def _read(self, name):
        try:
            with open(os.path.join(self.dir, name)) as f:
                return float(f.read().strip())
        except Exception:
            return None

    def read_sclk_mhz(self):
        """One reading of the shader clock (MHz), or None."""
        if self.dir is None:
            return None
        f = self._read("freq1_input")
        return None if f is None else round(f * 1e-6, 1)

    def _run(self):
        while not self._stop.is_set():
            p, f = self._read("power1_input"), self._read("freq1_input")
            if p is not None:
                self.power.append(p * 1e-6)
            if f is not None:
                self.freq.append(f * 1e-6)
            self._stop.wait(self.period)

    def start(self):
        if self.dir is not None:
            self._thread = threading.Thread(target=self._run, daemon=True)
            self._thread.start()

    def mark(self):
        """Forget what was sampled so far (the thread is started ahead of the region it is to cover)."""
        del self.power[:], self.freq[:]

    def stop(self):
        if self._thread is not None:
            self._stop.set()
            self._thread.join()

    def summary(self):
        if not self.power:
            return None
        cap = self._read("power1_cap")
        # the first samples still show the previous state of the averaging the SMU does: report the second half too
        half = self.power[len(self.power) // 2:]
        out = {"package_w_avg": round(sum(self.power) / len(self.power), 1), "package_w_last_half": round(sum(half) / len(half), 1),
               "package_w_max": round(max(self.power), 1), "cap_w": None if cap is None else round(cap * 1e-6, 1),
               "samples": len(self.power), "source": "amdgpu hwmon power1_input / freq1_input / power1_cap, polled every %g ms "
               "over the timed region" % (self.period * 1e3)}
        if self.freq:
            out["sclk_mhz_avg"] = round(sum(self.freq) / len(self.freq), 1)
            out["sclk_mhz_min"] = round(min(self.freq), 1)
        return out


def dump_outputs(out, out_dir, name="bscan_db"):
    """Writes the tensor `out` to out_dir/<name>.npy as float32: whole when it fits in DUMP_BYTES, else a sample of its rows
    (last dimension), the same for every run of the same shape (seed 0, rows in ascending order), as a (rows, out.shape[-1])
    array.  Returns the path."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    rows = out.reshape(-1, out.shape[-1])
    keep = DUMP_BYTES // (rows.shape[1] * 4)
    if rows.shape[0] > keep:
        sel = np.sort(np.random.default_rng(0).choice(rows.shape[0], keep, replace=False))
        out = rows[torch.from_numpy(sel).to(rows.device)]
    path = os.path.join(out_dir, name + ".npy")
    np.save(path, out.float().cpu().numpy())
    return path


def process_group_problems(ranks_seen, n_gpus, devices, share_gpu):
    """What makes an N > 1 line unusable as a scaling point: a process group that does not hold N ranks, or two ranks
    on one device (by PCI address) outside the --share-gpu rehearsal.  Returns a list of messages, empty when the group is sound."""
    problems = []
    if ranks_seen != n_gpus:
        problems.append("the process group holds %d ranks, --gpus says %d" % (ranks_seen, n_gpus))
    if n_gpus > 1 and not share_gpu:
        known = [d for d in devices if d]
        if len(devices) != n_gpus:
            problems.append("%d device entries for %d ranks" % (len(devices), n_gpus))
        if len(set(known)) != len(known):
            dup = sorted({d for d in known if known.count(d) > 1})
            problems.append("several ranks on one device (PCI %s): a scaling point needs one GPU per rank (--share-gpu is the rehearsal switch)" % ", ".join(dup))
    return problems


def self_launch(nproc):
    """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run --nproc-per-node N bench.py <same
    arguments>` as a child process (never an exec: this process may not replace itself once a GPU has been initialised, and
    keeping the rule unconditional is simpler), pass its stdout / stderr through and return its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: the workload's own, else 1000)")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: package power sampling, the CPU baselines, the parity check "
                         "against the oracle, the staged, half-chip, division-setting and sustained legs, the copy-rate ceilings")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the dB B-scans of the last timed step (rank 0) to DIR/bscan_db.npy, float32: all of them when they fit "
                         "in %d bytes, else a fixed seeded sample of rows (dump_outputs)" % DUMP_BYTES)
    ap.add_argument("--ramp-seconds", type=float, default=1.0,
                    help="untimed back-to-back steps run before the warmup so that the timed region starts in the SUSTAINED state: "
                         "memory / fabric clocks up (they need ~0.25 s of unbroken load) and the package at its power cap "
                         "(~1 s: before that the shader clock is still above its sustained level); see DESIGN.md 5, profiles/r05_ramp.txt")
    ap.add_argument("--workload", default="C2", choices=sorted(WORKLOADS))
    ap.add_argument("--frames-per-step", type=int, default=0, help="frames per step per GPU (0 = auto)")
    ap.add_argument("--ring", type=int, default=0, help="resident frames per GPU (0 = auto, >= 1 GiB)")
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic frames generated (tiled into the ring)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="with --full: seconds of the single-core CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--cpu-workers", type=int, default=16,
                    help="with --full: worker threads of the multi-core CPU figure (0 = every schedulable CPU; default 16 = a 1-GPU box's share)")
    ap.add_argument("--threads-per-block", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--plan", type=int, default=-1, help="FFT plan id (tuning; -1 = library default, -2 = the any-configuration kernel)")
    ap.add_argument("--general-kernel", action="store_true", help="force the predicated kernel (tuning)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend for --gpus > 1 (nccl = RCCL; gloo only for rehearsals without RCCL)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal: let all ranks use the same GPU (needs --backend gloo)")
    ap.add_argument("--input-bits", type=int, default=16, choices=[8, 16],
                    help="camera sample width: 16 (BASELINE's C2) or 8 (the shipped ini's cameras; not the headline)")
    ap.add_argument("--background-2d", action="store_true",
                    help="full H x W background frame (what the reference's 'b' key stores) instead of one spectrum: "
                         "+W*4 algorithmic bytes per A-scan, reported as its own mode (SURVEY 8d)")
    ap.add_argument("--stage-steps", type=int, default=50,
                    help="with --full: untimed two-kernel (resample stage, FFT stage) steps run AFTER the timed region so that the line "
                         "carries each stage's HBM roofline (0 = skip)")
    ap.add_argument("--half-chip-steps", type=int, default=200,
                    help="with --full: untimed steps on half of the compute units after the timed region: the per-clock rate below the power cap, "
                         "reported as `half_chip` (0 = skip)")
    ap.add_argument("--staged", action="store_true",
                    help="run the path as two kernels (resample stage, FFT stage) and report each stage's HBM roofline; "
                         "same results, 3x the traffic -- a measurement mode, not the headline configuration")
    ap.add_argument("--display-points", type=int, default=0,
                    help="numdisplaypoints override (tuning; 0 = the workload's own, which is what the metric is quoted on)")
    ap.add_argument("--lines-per-frame", type=int, default=0,
                    help="A-scans per frame override (tuning: store alignment of the D x H layout; 0 = the workload's own)")
    ap.add_argument("--layout", default="rowmajor", choices=["rowmajor", "transposed"],
                    help="output layout: rowmajor = H x D per B-scan (the headline); transposed = the reference's own D x H "
                         "`bscan` (main:1220), what the drop-in patch of INTEGRATION.md asks for -- reported as its own mode")
    ap.add_argument("--precise-division", action="store_true",
                    help="(the library default since round 5; kept so that older command lines still run)")
    ap.add_argument("--one-word-division", action="store_true",
                    help="time the run with the OPT-OUT fdoct_set_precise_division(h, 0): one f32 reciprocal of the background on the "
                         "fused fast path (outside the tolerance on fringes below ~1 %% of the DC level); reported as its own mode")
    ap.add_argument("--precise-steps", type=int, default=200,
                    help="with --full: untimed steps with the OTHER division setting after the timed region (the one-word opt-out next to the "
                         "default, or the default next to the opt-out), and the weak-fringe parity leg (fringes of 1e-3 of the DC "
                         "level against the oracle) with both settings, reported as `precise_division` (0 = skip)")
    ap.add_argument("--sustained-seconds", type=float, default=1.0,
                    help="with --full: untimed repetition of the SAME full launch after the timed region, long enough for the power sampler "
                         "(reported as `sustained`; 0 = skip)")
    args = ap.parse_args(argv)
    if args.steps is None:
        args.steps = WORKLOADS[args.workload].get("steps", 1000)
    return args


def main():
    args = parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # Invoked directly with --gpus N: start one rank per GPU as CHILD processes (torch.distributed.run) before anything
        # here has touched the GPU, relay their output (rank 0 prints the one JSON line) and exit with their code.
        raise SystemExit(self_launch(args.gpus))

    import torch
    import torch.distributed as dist
    from fdoct_amd import DTYPE_U8, DTYPE_U16, LAYOUT_ROWMAJOR, LAYOUT_TRANSPOSED, Config, Reconstructor, synth
    from fdoct_amd import dist as fdist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gpus_given = any(a == "--gpus" or a.startswith("--gpus=") for a in sys.argv[1:])
    if world != args.gpus and not gpus_given:
        # `torchrun --nproc-per-node N bench.py` without --gpus: the launcher's world size IS the GPU count; the
        # process-group check below still refuses anything that is not N ranks on N devices
        args.gpus = world
    if world != args.gpus:
        # an EXPLICIT --gpus that disagrees with the launcher: never a line that reads as an N-GPU result (exit code 3 on every rank)
        if rank == 0:
            sys.stderr.write("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE): refusing to run\n" % (args.gpus, world))
        raise SystemExit(3)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cdev = dev if args.backend == "nccl" else torch.device("cpu")  # where collective payloads live
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    # what the process group actually is: ranks it holds, the collective library, the PCI device of every rank
    group = {"ranks_seen": dist.get_world_size() if world > 1 else 1,
             "backend": (args.backend if world > 1 else None)}
    try:
        group["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:
        group["rccl_version"] = None
    try:
        my_bus = PowerSampler._pci_bus_id(local_rank)
    except Exception:
        my_bus = None
    if world > 1:
        buses = [None] * world
        dist.all_gather_object(buses, my_bus)
        group["devices"] = buses
    else:
        group["devices"] = [my_bus]
    # fail loudly, on every rank, before anything is timed: a group that is not N ranks on N devices is not a scaling point
    problems = process_group_problems(group["ranks_seen"], args.gpus, group["devices"], args.share_gpu)
    if problems:
        if rank == 0:
            sys.stderr.write("bench.py: unusable process group: " + "; ".join(problems) + "\n")
        if world > 1:
            dist.destroy_process_group()
        raise SystemExit(3)
    num_cu = torch.cuda.get_device_properties(dev).multi_processor_count

    wl = WORKLOADS[args.workload]
    if args.display_points:
        wl = dict(wl, D=args.display_points, desc=wl["desc"] + " [numdisplaypoints %d]" % args.display_points)
        WORKLOADS[args.workload] = wl
    if args.lines_per_frame:
        wl = dict(wl, H=args.lines_per_frame, desc=wl["desc"] + " [%d lines per frame]" % args.lines_per_frame)
        WORKLOADS[args.workload] = wl
    W, H, N, D, A = wl["W"], wl["H"], wl["N"], wl["D"], wl["A"]
    M, binv = wl.get("M", 1), wl.get("bin", 1)
    RW, RH = wl.get("raw_w", W), wl.get("raw_h", H)       # what the camera delivers: the kernels bin it (fdoct_set_frontend)
    if "bits" in wl:
        args.input_bits = wl["bits"]
    es = args.input_bits // 8
    frame_bytes = RW * RH * es
    fps = args.frames_per_step or wl.get("fps") or max(A, (1 << 30) // frame_bytes // A * A)     # ~1 GiB of input per step
    ring = args.ring or wl.get("ring") or 2 * fps                                # two steps' worth resident (2 GiB)
    ring = (ring + fps - 1) // fps * fps
    distinct = max(A, min(args.distinct, ring))

    lmin, lmax = wl.get("lmin", synth.LAMBDAMIN), wl.get("lmax", synth.LAMBDAMAX)
    cfg = Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, averages=A, device=local_rank,
                 increasefftpointsmultiplier=M, lambdamin=lmin, lambdamax=lmax)
    rec = Reconstructor(cfg)
    if binv > 1:
        rec.set_frontend(0, binv, binv)      # a run-time setting of the handle, not part of the broadcast state
    yb = synth.make_background(W)
    if es == 1:
        yb = np.maximum(yb >> 8, 1).astype(np.uint8)
    yb_set = np.ascontiguousarray(np.broadcast_to(yb, (H, W))) if args.background_2d else yb
    if rank == 0:
        rec.set_background(yb_set)
        if wl["hann"]:
            rec.set_window(synth.hann_window(W))
        if wl["phase"]:
            rec.set_dispersion_phase(synth.dispersion_phase(N))
        blob = rec.export_state()
    else:
        blob = None
    if world > 1:
        # set-up only: constant state from rank 0 over RCCL/xGMI; no data-path collective
        dist.barrier()
        t_bc = time.perf_counter()
        blob = fdist.broadcast_state(blob if rank == 0 else np.zeros(0, np.uint8), 0, cdev)
        if args.backend == "nccl":
            torch.cuda.synchronize()
        group["setup_broadcast"] = {"bytes": int(blob.size), "ms": round((time.perf_counter() - t_bc) * 1e3, 3),
                                    "how": "rank 0's wall clock around the two broadcasts (size, blob) incl. the copy back to the host; "
                                           "the first collective of a process group also sets the communicator up"}
        if rank != 0:
            rec.import_state(blob)
    if args.threads_per_block or args.blocks:
        rec.set_launch(args.threads_per_block, args.blocks)
    if args.plan != -1 or args.general_kernel:
        rec.set_plan(args.plan, args.general_kernel)
    if args.staged:
        rec.set_staged(True)
        rec.set_timing(True)   # per-stage device times come from the library's own events
    if os.environ.get("FDOCT_PRECISE_DIVISION", "") == "0":   # the library's own opt-out switch, honoured here too (tools/ab.sh)
        args.one_word_division = True
    timed_precise = not args.one_word_division     # the library default: both words of the reciprocal background
    rec.set_precise_division(timed_precise)

    # synthetic frames: each rank generates its own shard (different frame numbers), tiled into the ring
    f0 = rank * ring
    host = synth.make_frames(f0, distinct, RW, RH)                    # (distinct, RH, RW) u16: raw camera frames
    if es == 1:
        host = (host >> 8).astype(np.uint8)
        d_distinct = torch.from_numpy(host).to(dev)
    else:
        d_distinct = torch.from_numpy(host.view(np.int16)).to(dev)     # same bits; torch has no full u16 support
    reps = (ring + distinct - 1) // distinct
    d_ring = d_distinct.repeat(reps, 1, 1)[:ring].contiguous()
    transposed = args.layout == "transposed"
    layout = LAYOUT_TRANSPOSED if transposed else LAYOUT_ROWMAJOR
    d_out = torch.empty((fps // A, D, H) if transposed else (fps // A, H, D), dtype=torch.float32, device=dev)
    # a non-default torch stream: the library launches on it, and the torch events below see it
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rec.set_stream(stream.cuda_stream)
    pitch = RW * es
    in_dtype = DTYPE_U8 if es == 1 else DTYPE_U16
    nslots = ring // fps

    def step(i):
        off = (i % nslots) * fps
        rec.process_device(d_ring[off].data_ptr(), in_dtype, fps, pitch, None, d_out.data_ptr(), layout)

    if world > 1:
        dist.barrier()   # first collective sets up the communicator (seconds): not between warm-up and timing
    # Clock ramp: untimed launches before the W warmup steps, back to back -- the queue never runs empty (the host waits for the
    # burst before the last one, not for the last one), because the memory / fabric clocks that a sustained load raises fall back
    # within an idle gap: with a synchronize() after every burst, a driver-sized run (K = 20, a 10 ms timed region right after
    # the ramp) read 2-3 % below the K = 1000 run of the same box (round 5).
    ramp_steps = 0
    t_ramp = time.perf_counter()
    ramp_marks = []
    ramp_mode = os.environ.get("FDOCT_BENCH_RAMP", "continuous")      # "bursts": round 4's form, for the comparison in DESIGN.md
    while time.perf_counter() - t_ramp < args.ramp_seconds:
        for i in range(20):
            step(i)
        ramp_steps += 20
        if ramp_mode == "bursts":
            torch.cuda.synchronize()
            continue
        mark = torch.cuda.Event()
        mark.record(stream)
        ramp_marks.append(mark)
        if len(ramp_marks) > 2:
            ramp_marks.pop(0).synchronize()
    # everything the timed region needs exists before the warmup: nothing but the contract's synchronize() + barrier() lies
    # between the last warmup launch and the first timed one
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    psamp = PowerSampler(dev.index if dev.index is not None else 0) if rank == 0 and args.full else None
    if psamp is not None:
        psamp.start()
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    # device time of the timed region: one event pair on the launch stream around all K steps (an event pair per
    # step costs ~20 us of stream time per step, 4 % of this kernel); K launches / elapsed = average launch duration
    # including the ~2 us hand-over between consecutive launches
    torch.cuda.synchronize()
    if psamp is not None:
        psamp.mark()
    t0 = time.perf_counter()
    ev0.record(stream)
    for i in range(args.steps):
        step(args.warmup + i)
    ev1.record(stream)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if psamp is not None:
        psamp.stop()
    wall_elapsed = fdist.max_over_ranks(elapsed, cdev)
    if rank == 0 and args.dump_outputs:
        dump_outputs(d_out, args.dump_outputs)
    k_avg_ms = ev0.elapsed_time(ev1) / args.steps
    # what the timed launches ran on (fdoct_last_kernel): the label of the roofline object
    from fdoct_amd import capi as _capi
    kernel_label = {_capi.KERNEL_FUSED: "fused_kernel", _capi.KERNEL_FUSED_TRANSPOSED: "fused_kernel (transposed store)",
                    _capi.KERNEL_FUSED_STAGED: "resample kernel + FFT kernel (staged)",
                    _capi.KERNEL_WAVE: "wave_kernel", _capi.KERNEL_WAVE_JIT: "wave_kernel (compiled at run time)",
                    _capi.KERNEL_GENERIC: "generic_kernel",
                    _capi.KERNEL_LONG_ROWS: "big_pre + big_fft_group launches + big_post (whole launch sequence)"}.get(rec.last_kernel(), "?")
    if binv > 1:   # (the run-time compiled wave kernel takes the raw frames and bins in its loads; every other route bins in a pass of its own)
        kernel_label = ("wave_kernel (compiled at run time, 2 x 2 binning in its loads)" if rec.last_kernel() == _capi.KERNEL_WAVE_JIT
                        else "bin2x2_kernel + " + kernel_label)
    # `value` comes from DEVICE time: every rank times its own K launches with an event pair on its launch stream, and the
    # slowest rank's time is what the job took.  The wall clock around synchronize() + barrier() rides along as
    # `wall_ms_per_step`: with a driver-sized K the timed region is ~10 ms, and a few hundred microseconds of barrier / launch
    # skew between ranks would read as per cent of "scaling loss" that is not the path's.
    dev_elapsed = fdist.max_over_ranks(k_avg_ms * args.steps * 1e-3, cdev)
    elapsed = dev_elapsed
    per_rank = None
    try:
        my_sclk = PowerSampler(dev.index if dev.index is not None else 0).read_sclk_mhz()
    except Exception:
        my_sclk = None
    mine = {"rank": rank, "device_ms_per_step": round(k_avg_ms, 4), "ascans_per_s": round(fps * H / (k_avg_ms * 1e-3), 1),
            "pci_bus": my_bus, "sclk_mhz_after": my_sclk}
    if world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    else:
        per_rank = [mine]
    # Sustained power evidence: the timed region of the default run is ~0.5 s and of a short driver run a few ms -- too short
    # for the hwmon power average.  The SAME full launch repeats here, untimed (never part of `value` / `roofline`), for
    # --sustained-seconds with the sampler running.
    sustained = None
    if rank == 0 and args.full and args.sustained_seconds > 0:
        sps = PowerSampler(dev.index if dev.index is not None else 0)
        se0, se1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per_burst = max(1, int(0.02 / max(k_avg_ms * 1e-3, 1e-6)))      # ~20 ms of launches per host synchronisation
        sps.start()
        ts0 = time.perf_counter()
        se0.record(stream)
        nsus = 0
        while time.perf_counter() - ts0 < args.sustained_seconds:
            for i in range(per_burst):
                step(nsus + i)
            nsus += per_burst
            torch.cuda.synchronize()
        se1.record(stream)
        torch.cuda.synchronize()
        sps.stop()
        sms = se0.elapsed_time(se1)
        sustained = {"seconds": round(sms * 1e-3, 3), "steps": nsus, "ascans_per_s": round(nsus * fps * H / (sms * 1e-3), 1),
                     "how": "the timed launch repeated after the timed region, untimed, with the hwmon sampler running"}
        sustained.update(sps.summary() or {})
        step(args.warmup + args.steps - 1)               # the last timed step's output again, for the parity check below
        torch.cuda.synchronize()
    stages = None
    stages_note = None
    # per-stage roofline (north star: "rocprof must show achieved HBM GB/s ... for the resample and FFT stages"): the same
    # chain as two kernels with the k-linear rows in HBM between them.  In the default (fused) mode these are UNTIMED
    # extra steps after the timed region; `value` and `roofline` above never include them.
    can_stage = (fps <= 2048 and es == 2 and not args.general_kernel and not args.background_2d and not transposed and M == 1 and binv == 1)
    want_stages = args.staged or (args.full and args.stage_steps > 0 and rank == 0)
    if want_stages and not can_stage:
        stages_note = ("staged kernels exist for the plain u16, row-major configuration only" if fps <= 2048 else
                       "no staged steps at this batch size (the k-linear rows of a %d-frame step would take %.0f GB); see the C2 line" % (fps, fps * H * N * 4 / 1e9))
    if want_stages and can_stage:
        # per-stage device times from the library's own HIP events on the launch stream
        if not args.staged:
            rec.set_staged(True)
            rec.set_timing(True)
        nst = min(args.steps, 10) if args.staged else args.stage_steps
        r_ms, f_ms = [], []
        try:
            for i in range(nst + (0 if args.staged else 5)):
                step(args.warmup + args.steps - 1)  # the slot of the last timed step (the parity check reads its output)
                t = rec.timing()
                if args.staged or i >= 5:               # (first steps: workspace allocation, clock)
                    r_ms.append(t["resample_stage_ms"])
                    f_ms.append(t["fft_stage_ms"])
        except Exception as e:  # e.g. no memory for the intermediate rows: report, keep the headline
            stages_note = "staged steps failed: %s" % str(e)[:120]
            r_ms = f_ms = []
        if not args.staged:
            rec.set_staged(False)
            rec.set_timing(False)
            torch.cuda.synchronize()
            step(args.warmup + args.steps - 1)           # the fused chain's output again, for the parity check below
            torch.cuda.synchronize()
    # What the chain does per clock, away from the package power cap: the same launch on HALF the compute units
    # (one workgroup per CU, 128 of 256), untimed extra steps after the timed region, with the power / clock of those steps.
    # `value` and `roofline` above never include them.
    half_chip = None
    if rank == 0 and args.full and args.half_chip_steps > 0 and not args.blocks and not args.staged and not transposed:
        try:
            hb = max(1, num_cu // 2)
            rec.set_launch(args.threads_per_block, hb)
            for i in range(20):
                step(args.warmup + args.steps - 1)
            torch.cuda.synchronize()
            hps = PowerSampler(dev.index if dev.index is not None else 0)
            he0, he1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hps.start()
            he0.record(stream)
            for i in range(args.half_chip_steps):
                step(args.warmup + args.steps - 1)
            he1.record(stream)
            torch.cuda.synchronize()
            hps.stop()
            hms = he0.elapsed_time(he1) / args.half_chip_steps
            hrate = fps * H / (hms * 1e-3)
            hbytes = RW * binv * es + D * 4 / A
            half_chip = {"workgroups": hb, "steps": args.half_chip_steps, "kernel_ms_avg": round(hms, 4), "ascans_per_s": round(hrate, 1),
                         "ascans_per_s_per_workgroup": round(hrate / hb, 1),
                         "whole_chip_at_this_rate": {"ascans_per_s": round(hrate / hb * num_cu, 1), "compute_units": num_cu,
                                                     "frac_of_hbm_peak": round(hrate / hb * num_cu * hbytes / 1e9 / HBM_PEAK_GBS, 4)},
                         "power": hps.summary(),
                         "how": "the timed launch restricted to one workgroup on half of the compute units (fdoct_set_launch), untimed steps after the timed region"}
        except Exception as e:
            half_chip = {"failed": str(e)[:120]}
        rec.set_launch(args.threads_per_block, args.blocks)
        torch.cuda.synchronize()
        step(args.warmup + args.steps - 1)           # the full launch's output again, for the parity check below
        torch.cuda.synchronize()
    # The division by the background in more than one float (fdoct_set_precise_division): what it costs on this
    # workload -- the same launch with it on, untimed extra steps after the timed region -- and what it buys: frames whose
    # fringes are 1e-3 of the DC level (a sample arm's return, not the synthetic mirror pair of the timed frames) against the
    # oracle, with the SURVEY tolerance.  `value` and `roofline` never include these steps.
    precise = None
    if rank == 0 and args.full and args.precise_steps > 0 and not args.staged:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import helpers
            rec.set_precise_division(not timed_precise)
            for i in range(20):
                step(args.warmup + args.steps - 1)
            torch.cuda.synchronize()
            pe0, pe1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pe0.record(stream)
            for i in range(args.precise_steps):
                step(args.warmup + args.steps - 1)
            pe1.record(stream)
            torch.cuda.synchronize()
            pms = pe0.elapsed_time(pe1) / args.precise_steps
            prate = fps * H / (pms * 1e-3)
            pbytes = RW * binv * es + D * 4 / A
            other = {"steps": args.precise_steps, "kernel_ms_avg": round(pms, 4), "ascans_per_s": round(prate, 1),
                     "frac_of_hbm_peak": round(prate * pbytes / 1e9 / HBM_PEAK_GBS, 4),
                     "rate_vs_timed_region": round(prate / (fps * H / (k_avg_ms * 1e-3)), 4),
                     "how": "the timed launch with fdoct_set_precise_division(h, %d), untimed steps after the timed region" % (0 if timed_precise else 1)}
            precise = {"timed_region": "both words of 1/background (the library default, main:1132 divides in double)" if timed_precise
                                       else "one word (the opt-out, fdoct_set_precise_division(h, 0))",
                       ("one_word_opt_out" if timed_precise else "both_words_default"): other}
            # weak-fringe parity leg, both settings
            amp, rows = 1e-3, 8
            wdt = np.uint8 if es == 1 else np.uint16
            wfr = np.concatenate([synth.weak_fringe_frame(amp, RW, RH, seed=5 + a_, dtype=wdt)[0] for a_ in range(A)])
            ofr = wfr[:, :rows * binv]
            if binv > 1:
                import oracle_lib as orc_fe
                ofr = np.stack([orc_fe.resize_area(f, binv, binv) for f in ofr]).astype(wdt)
            ocfg = Config(width=W, height=rows, numfftpoints=N, numdisplaypoints=D, averages=A, increasefftpointsmultiplier=M,
                          lambdamin=lmin, lambdamax=lmax)
            mag_o, _, db_o = helpers.oracle_reference(
                ocfg, ofr, yb, window=synth.hann_window(W) if wl["hann"] else None,
                phase=synth.dispersion_phase(N) if wl["phase"] else None)
            mag_tw = helpers.oracle_truth(ocfg, ofr, yb, window=synth.hann_window(W) if wl["hann"] else None,
                                          phase=synth.dispersion_phase(N) if wl["phase"] else None)[0]
            leg = {"fringe_amplitude_of_dc": amp, "rows": rows}
            for name, on in (("on", True), ("off", False)):
                rec.set_precise_division(on)
                bw, _ = rec.process(wfr, want_db=False)
                leg["worst_err_over_tol_" + name] = round(float(helpers.mag_ratio(bw[:, :rows], mag_o).max()), 4)
                leg["vs_truth_" + name] = round(helpers.truth_ratios(bw[:, :rows], mag_tw)[0], 4)
            leg["vs_truth_f32_oracle"] = round(helpers.truth_ratios(mag_o, mag_tw)[0], 4)
            leg["timed_configuration"] = leg["worst_err_over_tol_on" if timed_precise else "worst_err_over_tol_off"]
            precise["weak_fringe_parity"] = leg
        except Exception as e:  # report, do not hide
            precise = dict(precise or {}, failed=str(e)[:200])
        rec.set_precise_division(timed_precise)
        rec.set_stream(stream.cuda_stream)
        torch.cuda.synchronize()
        step(args.warmup + args.steps - 1)           # the timed configuration's output again, for the parity check below
        torch.cuda.synchronize()
    if want_stages and can_stage and r_ms:
        nin = fps * H
        # per-stage algorithmic bytes: resample = W*2 in + N*4 out; FFT+mag+log = N*4 in + D*4 out
        # (complex path: N*8 for the intermediate)
        inter = N * (8 if wl["phase"] else 4)
        for name, ms, nbytes in (("resample", float(np.mean(r_ms)), W * es + inter), ("fft_mag_log", float(np.mean(f_ms)), inter + D * 4 / A)):
            gbs = nbytes * nin / (ms * 1e-3) / 1e9
            stages = (stages or []) + [{"stage": name, "kernel_ms_avg": round(ms, 4), "kernel_ms_min": round(float(np.min(r_ms if name == "resample" else f_ms)), 4),
                                        "launches": len(r_ms), "algorithmic_bytes_per_ascan": nbytes,
                                        "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                        "frac": round(gbs / HBM_PEAK_GBS, 4)}]

    ascans_step = fps * H                                # input A-scans per step per GPU
    total_ascans = ascans_step * args.steps * world
    value = total_ascans / elapsed
    # algorithmic bytes per A-scan: W*b_in in + D*4/A out
    # (a full-frame background adds W*4 B per A-scan of reads that L2 / Infinity Cache serve: reported, not counted as HBM)
    bytes_per_ascan = RW * binv * es + D * 4 / A      # one input A-scan = binv raw rows of RW samples
    if args.staged:  # the intermediate k-linear rows are written and read once more
        bytes_per_ascan += 2 * N * (8 if wl["phase"] else 4)   # (per input A-scan, also with averaging)
    bytes_launch = bytes_per_ascan * ascans_step
    achieved = bytes_launch / (k_avg_ms * 1e-3) / 1e9

    # parity spot check of the timed configuration (rank 0): first rows of the last batch vs the oracle
    parity = None
    cpu = None
    if rank == 0 and args.full:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import helpers
            rows = 8
            last = (args.warmup + args.steps - 1) % nslots * fps
            fr = d_ring[last:last + A, :rows * binv].cpu().numpy()
            fr = fr if es == 1 else fr.view(np.uint16)
            if binv > 1:
                import oracle_lib as orc_fe
                fr = np.stack([orc_fe.resize_area(f, binv, binv) for f in fr]).astype(fr.dtype)
            got = (d_out[0, :, :rows].t().contiguous() if transposed else d_out[0, :rows]).cpu().numpy()
            ocfg = Config(width=W, height=rows, numfftpoints=N, numdisplaypoints=D, averages=A, increasefftpointsmultiplier=M,
                          lambdamin=lmin, lambdamax=lmax)
            mag_o, _, db_o = helpers.oracle_reference(
                ocfg, fr, yb, window=synth.hann_window(W) if wl["hann"] else None,
                phase=synth.dispersion_phase(N) if wl["phase"] else None)
            db_rm = np.transpose(db_o, (0, 2, 1))
            rate, worst_db, nb = helpers.db_flat_pass_rate(got[None], db_rm, mag_o)
            parity = {"rows": rows, "flat_1e-3_dB_pass_rate": round(rate, 6), "max_abs_db_above_1e-4_rowmax": round(worst_db, 6),
                      "bins_counted": nb}
            # Adjudication against the reference's MATHEMATICS (the chain in double, oracle_truth) next to the comparison with the
            # f32 restatement: the timed launch's dB image, and -- from one more, untimed, call on the same frames -- the linear one
            mag_t, _, db_t = helpers.oracle_truth(
                ocfg, fr, yb, window=synth.hann_window(W) if wl["hann"] else None,
                phase=synth.dispersion_phase(N) if wl["phase"] else None)
            db_t_rm = np.transpose(db_t, (0, 2, 1))
            truth = {"what": "|x - truth| / tolerance, truth = the reference chain evaluated in double on the same frames and tables "
                             "(oracle/fdoct_oracle.h, orc_params.truth); limit for the HIP result: max(0.5, the f32 restatement's own)",
                     "db_gpu": round(float(helpers.db_ratio(got[None], db_t_rm, mag_t).max()), 4),
                     "db_f32_oracle": round(float(helpers.db_ratio(db_rm, db_t_rm, mag_t).max()), 4)}
            try:
                if args.precise_steps <= 0:   # (the counter passes of tools/prof_round.sh: no extra launch of the timed kernel)
                    raise RuntimeError("skipped with --precise-steps 0 (one more launch of the timed kernel on A frames)")
                full = d_ring[last:last + A].cpu().numpy()
                full = full if es == 1 else full.view(np.uint16)
                lin, _ = rec.process(full, want_db=False)
                g_lin, o_lin = helpers.truth_ratios(lin[:, :rows], mag_t, mag_o)
                truth.update(linear_gpu=round(g_lin, 4), linear_f32_oracle=round(o_lin, 4),
                             within_limit=bool(g_lin <= max(helpers.TRUTH_LIMIT, o_lin) and truth["db_gpu"] <= max(helpers.TRUTH_LIMIT, truth["db_f32_oracle"])))
            except Exception as e:  # report, do not hide
                truth["linear_failed"] = str(e)[:160]
            parity["truth"] = truth
            worst = helpers.check_db(got[None], db_rm, mag_o, "bench parity")
            parity["worst_db_err_over_tol"] = round(float(worst), 4)
        except AssertionError as e:  # report, do not hide
            parity = dict(parity or {}, failed=str(e)[:200])
        if not args.no_cpu_baseline and world == 1:
            host16, yb16 = host.astype(np.uint16), yb.astype(np.uint16)
            med, best, nfr = cpu_baseline(wl, host16, yb16, args.cpu_seconds, 1)
            cpu = {"value": round(med, 1), "unit": "A-scans/s", "cores": 1, "kind": "port",
                   "sample": "%d frames of the same %dx%d workload (16-bit containers) through oracle/%s (median of per-call rates, best %.0f)"
                             % (nfr, RW, RH, " incl. the software binning" if binv > 1 else "", best),
                   "host_cpus": os.cpu_count(), "host_cpu_model": _cpu_model()}
            try:
                navail = len(os.sched_getaffinity(0))
            except AttributeError:
                navail = os.cpu_count() or 1
            ncore = min(navail, args.cpu_workers) if args.cpu_workers > 0 else navail
            rate_mt, nfr_mt = cpu_baseline_frames_parallel(wl, host16, yb16, max(3.0, args.cpu_seconds / 2), ncore)
            cpu["multi_core"] = {"value": round(rate_mt, 1), "cores": ncore, "sample_frames": nfr_mt,
                                 "how": "one single-threaded frame chain per worker thread, frames in parallel; workers = "
                                        "min(schedulable CPUs, --cpu-workers): a 1-GPU box's CPU share is 16 of the host's cores"}

    # context for the roofline fraction: the device-to-device copy rate this GPU reaches right now, and
    # the FFT arithmetic rate (5 N log2 N per complex transform, half of it for real rows)
    copy_gbs = copy_f4 = copy_f4_note = None
    if rank == 0 and args.full:
        src_t = d_ring.view(torch.uint8).reshape(-1)
        dst_t = torch.empty_like(src_t[: min(src_t.numel(), 1 << 30)])
        ce0, ce1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            for _ in range(3):
                dst_t.copy_(src_t[: dst_t.numel()])
            ce0.record(stream)
            for _ in range(10):
                dst_t.copy_(src_t[: dst_t.numel()])
            ce1.record(stream)
        torch.cuda.synchronize()
        copy_gbs = 2.0 * dst_t.numel() * 10 / (ce0.elapsed_time(ce1) * 1e-3) / 1e9
        # ... and the in-tree 16-bytes-per-lane copy kernel (tools/ubench/copy_f4.hip): the access pattern the micro-architecture
        # guide quotes at 6.29 TB/s.  torch's copy_ reaches ~5.2 TB/s on this image and flatters a fraction taken against it.
        copy_f4 = copy_f4_note = None
        try:
            import ctypes
            so = os.path.join(ROOT, "tools", "ubench", "libcopy_f4.so")
            cl = ctypes.CDLL(so)
            cl.copy_f4.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
            nb = dst_t.numel() // 16 * 16
            copy_f4 = {}
            for vname, variant in (("plain", 0), ("nontemporal", 1)):
                for _ in range(3):
                    rc = cl.copy_f4(dst_t.data_ptr(), src_t.data_ptr(), nb, variant, 0, stream.cuda_stream)
                    assert rc == 0, rc
                ce0.record(stream)
                for _ in range(10):
                    cl.copy_f4(dst_t.data_ptr(), src_t.data_ptr(), nb, variant, 0, stream.cuda_stream)
                ce1.record(stream)
                torch.cuda.synchronize()
                copy_f4[vname] = 2.0 * nb * 10 / (ce0.elapsed_time(ce1) * 1e-3) / 1e9
            assert torch.equal(dst_t[:nb], src_t[:nb])
        except Exception as e:  # the ceiling is context, not the measurement: report why it is missing
            copy_f4, copy_f4_note = None, str(e)[:160]
        del dst_t
    fft_flops = (5.0 if wl["phase"] else 2.5) * N * np.log2(N)
    if M > 1:   # zero-pad stage: forward W-point and inverse M*W-point real transforms (main:211, 241)
        fft_flops += 2.5 * W * np.log2(W) + 2.5 * M * W * np.log2(M * W)
    fft_tflops = fft_flops * ascans_step / (k_avg_ms * 1e-3) / 1e12

    traffic = None
    traffic_source = None
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic_transposed.json" if transposed else "pmc_traffic.json")
    if os.path.exists(tpath):
        try:
            t = json.load(open(tpath))
            default_mode = not (args.staged or args.display_points or args.lines_per_frame or args.background_2d or es == 1 or args.general_kernel or args.plan != -1)
            if default_mode and t.get("workload") == args.workload and t.get("frames_per_step") == fps:
                traffic = t.get("hbm_bytes_per_launch")
                traffic_source = "profiles/%s (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE of this command, %s; not re-measured in this run)" % (os.path.basename(tpath), t.get("tag", "committed"))
        except Exception:
            traffic = None

    if rank == 0:
        power = psamp.summary() if psamp is not None else None
        if power and world == 1:
            power["ascans_per_joule"] = round(value / power["package_w_last_half"], 1)   # the quantity the cap bounds
        out = {
            "metric": {"C1": "A-scans/sec (1024-pt, 512 lines/frame)", "C4": "A-scans/sec (4096-pt, 2048 lines/frame, avg 16)",
                       "INI": "input A-scans/sec (160 samples x4 zero-pad -> 2560-pt, 120 lines/frame, avg 10, raw 320x240 u8 frames)",
                       "LONG": "A-scans/sec (4096 samples x8 zero-pad -> 32768-pt, 64 lines/frame)",
                       "LONG4": "A-scans/sec (4096 samples x4 zero-pad -> 16384-pt, 64 lines/frame)"}.get(
                args.workload, "A-scans/sec (2048-pt, 1000 lines/frame)"),
            "value": round(value, 1), "unit": "A-scans/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "wall_ms_per_step": round(wall_elapsed / args.steps * 1e3, 4),
            "value_wall": round(total_ascans / wall_elapsed, 1), "timing_version": 2,
            "timing": "value = A-scans of all ranks / MAX over ranks of the device time of the K launches (one HIP event pair per rank on its "
                      "launch stream); wall_ms_per_step = MAX over ranks of the host clock around synchronize() + barrier()",
            "per_rank": per_rank, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s: %s" % (args.workload, wl["desc"] if es == 2 else wl["desc"].replace("u16", "u8")), "width": W, "lines_per_frame": H,
                       "raw_frame": [RH, RW], "binvalue": binv, "increasefftpointsmultiplier": M, "numfftpoints": N, "numdisplaypoints": D, "averages": A, "input": "u%d" % args.input_bits, "output": "dB f32 DxH (the reference's bscan layout)" if transposed else "dB f32 HxD",
                       "frames_per_step_per_gpu": fps, "resident_ring_frames_per_gpu": ring, "parallelism": "frame-shard x%d" % world,
                       "clock_ramp_steps": ramp_steps},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": kernel_label, "kernel_ms_avg": round(k_avg_ms, 4),
                         "algorithmic_bytes_per_ascan": bytes_per_ascan, "ascans_per_launch": ascans_step,
                         "measured_copy_gbs": round(copy_gbs, 1) if copy_gbs else None,
                         "frac_of_measured_copy": round(achieved / copy_gbs, 4) if copy_gbs else None,
                         "measured_copy_how": "torch.Tensor.copy_ of 1 GiB, read + write bytes (kept for continuity with rounds 1-5; it is NOT the "
                                              "chip's copy ceiling: see achievable)",
                         # the honest second denominator: the guide's achievable HBM rate (float4 copy, read + write) and the same
                         # pattern measured on THIS card by the in-tree kernel
                         "achievable_guide_gbs": HBM_ACHIEVABLE_GBS,
                         "frac_of_achievable": round(achieved / HBM_ACHIEVABLE_GBS, 4),
                         "copy_f4_gbs": {k: round(v, 1) for k, v in copy_f4.items()} if copy_f4 else None,
                         "frac_of_copy_f4": round(achieved / max(copy_f4.values()), 4) if copy_f4 else None,
                         "copy_f4_how": copy_f4_note or "tools/ubench/copy_f4.hip: 16 B per lane, 1 GiB device-to-device, read + write bytes over 10 launches, best of plain / non-temporal",
                         "fft_tflops_f32": round(fft_tflops, 2)},
            "power": power,
            "sustained": sustained,
            "cpu_baseline": cpu,
            "parity": parity,
            "precise_division": precise,
            "process_group": group,
        }
        if world > 1 and args.full:
            out["cpu_baseline_note"] = "the CPU baseline is timed at N = 1 only (rank 0 of a one-GPU run)"
        # Second ceilings (every BASELINE workload sits at the package power cap, so HBM bandwidth alone mis-prices
        # the instruction-heavy ones).  (1) package power: what this run drew against the cap, the energy per input A-scan and
        # its split into the always-on floor, the HBM share (bytes x the measured energy per byte) and the on-chip rest;
        # (2) FP32 vector rate of the DFT arithmetic alone against the 157.3 TFLOP/s vector peak.
        pw = sustained if (sustained and sustained.get("package_w_avg")) else power
        if pw and pw.get("package_w_avg") and world == 1:
            P = pw.get("package_w_last_half") or pw["package_w_avg"]
            cap = pw.get("cap_w") or 1400.0
            rate = (sustained or {}).get("ascans_per_s") or value
            uj = P / rate * 1e6
            floor_w, pj_per_hbm_byte = 347.0, 100.0     # profiles/r02_power_probe.txt: all wave slots idle-looping; read+write stream
            uj_floor, uj_hbm = floor_w / rate * 1e6, bytes_per_ascan * pj_per_hbm_byte * 1e-6
            out["roofline_power"] = {"bound": "package_power", "achieved": round(P, 1), "peak": cap, "unit": "W", "frac": round(P / cap, 4),
                                     "uj_per_ascan": round(uj, 4), "uj_floor": round(uj_floor, 4), "uj_hbm": round(uj_hbm, 4),
                                     "uj_onchip": round(uj - uj_floor - uj_hbm, 4),
                                     "ascans_per_s_at_the_cap_with_this_energy": round(rate * cap / P, 1),
                                     "ascans_per_s_at_the_cap_if_only_hbm_energy": round((cap - floor_w) / (uj_hbm * 1e-6), 1),
                                     "source": "hwmon power of the %s; floor %.0f W and %.0f pJ per HBM byte from profiles/r02_power_probe.txt"
                                               % ("sustained repetition" if pw is sustained else "timed region", floor_w, pj_per_hbm_byte)}
        out["roofline_fp32"] = {"bound": "fp32_valu", "achieved": round(fft_tflops, 2), "peak": 157.3, "unit": "TFLOP/s",
                                "frac": round(fft_tflops / 157.3, 4),
                                "counts": "DFT arithmetic only (5 N log2 N per complex transform, half for real rows)"}
        if args.workload == "INI":
            # 768 algorithmic bytes per A-scan: HBM is not what bounds these short rows; the binding resources
            # are the LDS pipe and VALU issue.  Per-A-scan counter figures from the committed PMC run, clock from this run.
            onchip = {"bound": "lds_pipe / valu_issue", "note": "HBM fraction above is not the binding ceiling for this workload"}
            ipath = os.path.join(ROOT, "profiles", "pmc_ini.json")
            sclk = (power or {}).get("sclk_mhz_avg") or ((sustained or {}).get("sclk_mhz_avg"))
            if os.path.exists(ipath) and sclk and world == 1:
                pj = json.load(open(ipath))
                cyc = sclk * 1e6 * num_cu / value            # CU-cycles the chip spends per input A-scan
                onchip.update({"cu_cycles_per_ascan": round(cyc, 1), "sclk_mhz": sclk,
                               "lds_active_cycles_per_ascan": pj["lds_active_cycles_per_ascan"],
                               "lds_pipe_busy_frac": round(pj["lds_active_cycles_per_ascan"] / cyc, 4),
                               "valu_insts_per_ascan": pj["valu_insts_per_ascan"],
                               # a 64-lane VALU instruction holds its 16-lane SIMD for 4 cycles; 4 SIMDs per CU
                               "valu_busy_frac": round(pj["valu_insts_per_ascan"] * 4.0 / (4.0 * cyc), 4),
                               "counters_source": "profiles/pmc_ini.json (%s; not re-measured in this run)" % pj.get("tag")})
            out["onchip"] = onchip
        if transposed:
            out["mode"] = "transposed output (D x H per B-scan, BscanFFT.cpp:1220); the row-major layout is the headline configuration"
            chain_writes = kernel_label.startswith("fused_kernel (transposed store)")   # (fdoct_last_kernel right behind the timed launches)
            out["roofline"]["kernel"] = ("fused_kernel, TRO instantiation (the chain writes D x H itself: LDS ring / in-place tiles); "
                                         "FDOCT_NO_TRO=1 selects the two-pass path fused_kernel + transpose64_kernel") if chain_writes else (
                                         kernel_label + " + transpose64_kernel (two passes: this plan has no transposed store of its own)")
            out["roofline"]["kernel_ms_avg_is"] = "device time per step: every launch of the step"
            if chain_writes:
                # what the memory system sustains for this layout's stores with nothing to compute (tools/ubench/rw_mix, 4 KB read + 4 KB
                # written per row and wave, reads + writes): 64-byte segments (tiles of 16 A-scans) against 5.15 TB/s with row-major stores
                out["roofline"]["pattern_ceiling_gbs"] = 3680.0
                out["roofline"]["pattern_ceiling_source"] = "profiles/r06_rw_mix.txt (measured at 1:1 read:write; not re-measured in this run)"
                out["roofline"]["frac_of_pattern_ceiling"] = round(out["roofline"]["achieved"] / 3680.0, 4)
        if args.one_word_division:
            out["mode"] = "one-word division (the opt-out fdoct_set_precise_division(h, 0)); the default multiplies by both words of 1/background"
        if args.background_2d:
            out["mode"] = "2-D background frame (+W*4 B per A-scan of reciprocal-background reads, served by L2 / Infinity Cache)"
            out["roofline"]["cached_background_bytes_per_ascan"] = W * 4
        if args.staged and stages:
            out["mode"] = "staged (two kernels; the default fused chain is the headline configuration)"
            out["roofline"]["kernel"] = "resample stage + FFT stage"
        if half_chip:
            out["half_chip"] = half_chip
        if stages:
            out["stages"] = stages
            if not args.staged:
                out["stages_how"] = ("%d untimed two-kernel steps after the timed region (fdoct_set_staged): same results bit for bit, "
                                     "the k-linear rows cross HBM between the stages; device time per stage from HIP events on the launch stream"
                                     % args.stage_steps)
        elif stages_note:
            out["stages"] = None
            out["stages_note"] = stages_note
        print(json.dumps(out))
    rec.close()
    if world > 1:
        dist.barrier()   # rank 0 ran the untimed extras (sustained power, stages, half chip): leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
