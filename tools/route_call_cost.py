"""Host time of one fdoct_process_async call: 10 000 back-to-back calls of one 8-row B-scan on a fused shape and on a built-in
wave-per-row shape, timed on the host from the first call to the return of the last, one synchronisation after the clock has
stopped.  The route is decided on the host in every call, so this is where a change of choose_route would show.  One line per shape:
nanoseconds per call.  Run it several times per library (FDOCT_LIB) and compare medians (profiles/route_value_cost.txt).
usage: python tools/route_call_cost.py [calls]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fdoct_amd import capi  # noqa: E402
from fdoct_amd.capi import Config, Reconstructor  # noqa: E402

H = 8
SHAPES = [("fused 2048x1->2048", 2048, 1, 2048, 1024), ("wave 640x4->2560", 640, 4, 2560, 320)]


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    for name, W, M, N, D in SHAPES:
        rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, device=0))
        rec.set_background(np.full(W, 1000.0))
        frames = torch.from_numpy(np.random.default_rng(0).integers(500, 1500, (1, H, W)).astype(np.int16)).cuda()  # (16-bit samples)
        mag = torch.empty((1, H, D), dtype=torch.float32, device="cuda")
        db = torch.empty_like(mag)
        fam = rec.prepare(capi.DTYPE_U16)
        args = (rec.h, frames.data_ptr(), capi.DTYPE_U16, 1, 0, mag.data_ptr(), db.data_ptr(), capi.LAYOUT_ROWMAJOR)
        call = rec.lib.fdoct_process_async
        for _ in range(500):
            assert call(*args) == 0
        rec.synchronize()
        t0 = time.perf_counter_ns()
        for _ in range(calls):
            call(*args)
        t1 = time.perf_counter_ns()
        rec.synchronize()
        assert rec.last_kernel() == fam and torch.isfinite(mag).all()
        print("%s: family %d, %d calls, %.1f ns per call" % (name, fam, calls, (t1 - t0) / calls), flush=True)
        rec.close()


if __name__ == "__main__":
    main()
