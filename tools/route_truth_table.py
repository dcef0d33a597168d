"""What fdoct_prepare answers over the grid of tests/native/route_check.cpp, as far as the public API expresses it: for every shape
and option one line with the returned kernel family (or the error code and fdoct_last_error) and fdoct_jit_note where it is not empty.  For refactors of the
route: run it once with FDOCT_LIB at the parent commit's library and once at the branch's (one process each) and compare the two
outputs -- they must be identical (profiles/route_value_truth_table.txt).  Creates handles and calls fdoct_prepare only: no frames,
no launch.  Not expressible through fdoct_prepare, hence not here: addresses and pitches off the vector grids, many B-scans, block
overrides per call, the complex call.  One built-in wave shape takes every option, the others those whose route depends on the
shape.
usage: python tools/route_truth_table.py > table.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fdoct_amd import capi  # noqa: E402
from fdoct_amd.capi import Config, Reconstructor  # noqa: E402

# route_check.cpp's shapes (W, M, N, D) and the in-kernel binning's edges
SHAPES = [(1024, 1, 1024, 512), (2048, 1, 2048, 1024), (160, 4, 2560, 320), (640, 4, 2560, 320), (720, 4, 2880, 360),
          (640, 1, 640, 320), (192, 4, 2560, 320), (1280, 1, 1280, 640), (321, 4, 2048, 512), (640, 1, 1400, 320),
          (4096, 1, 131072, 2048)]
BIN_EDGES = [(320, 4, 2560, 320), (336, 4, 2560, 320), (384, 4, 2560, 320)]
H = 8
FAMILY = ["none", "fused", "fused_transposed", "fused_staged", "wave", "wave_jit", "generic", "long_rows"]
U8, U16, F32, F64 = capi.DTYPE_U8, capi.DTYPE_U16, capi.DTYPE_F32, capi.DTYPE_F64
FULL = {(640, 4, 2560, 320)}   # every option; the other shapes take CORE's
CORE = {"base", "u8", "f32", "phase", "deep", "bin2x2", "DxH", "staged", "pi", "jit=0 pi"}


def option(label, dtype=U16, layout=capi.LAYOUT_ROWMAJOR, cfg=None, setup=None):
    return label, dtype, layout, cfg or {}, setup or (lambda r, s: None)


def phase(r, s):
    a = np.linspace(0.0, 1.0, s[2])
    r.set_dispersion_phase(np.stack([np.cos(a), np.sin(a)], axis=1))


OPTIONS = [
    option("base"), option("u8", U8), option("f32", F32), option("f64", F64),
    option("pi", setup=lambda r, s: r.set_pi_frame(np.full(s[0], 10.0))),
    option("dark", setup=lambda r, s: r.set_dark(np.full(s[0], 3.0))),
    option("bandpass", setup=lambda r, s: r.set_bandpass(True)),
    option("rownorm", cfg=dict(rowwisenormalize=1)),
    option("framenorm", cfg=dict(donotnormalize=0)),
    option("rownorm+normalize", cfg=dict(rowwisenormalize=1, donotnormalize=0)),
    option("sim variant", cfg=dict(variant=capi.VARIANT_SIM)),
    option("phase", setup=phase),
    option("deep", cfg=dict(deep=True)),
    option("bg=2d", setup=lambda r, s: r.set_background(np.full((H, s[0]), 1000.0))),
    option("movavg u8", U8, cfg=dict(movavgn=5)), option("movavg u16", U16, cfg=dict(movavgn=5)),
    option("movavg f32", F32, cfg=dict(movavgn=5)), option("movavg f64", F64, cfg=dict(movavgn=5)),
    option("median3", setup=lambda r, s: r.set_frontend(3, 1, 1)),
    option("median7 u8", U8, setup=lambda r, s: r.set_frontend(7, 1, 1)),
    option("median7 u16", setup=lambda r, s: r.set_frontend(7, 1, 1)),
    option("bin2x2", setup=lambda r, s: r.set_frontend(0, 2, 2)),
    option("bin2x2 u8", U8, setup=lambda r, s: r.set_frontend(0, 2, 2)),
    option("bin2x2 framenorm", cfg=dict(donotnormalize=0), setup=lambda r, s: r.set_frontend(0, 2, 2)),
    option("bin2x2 median3", setup=lambda r, s: r.set_frontend(3, 2, 2)),
    option("bin2x2 jit=0", setup=lambda r, s: (r.set_frontend(0, 2, 2), r.set_jit(False))),
    option("bin4x4", setup=lambda r, s: r.set_frontend(0, 4, 4)),
    option("bin2x2 f32", F32, setup=lambda r, s: r.set_frontend(0, 2, 2)),
] + [option("colour%d" % ch, U8, setup=lambda r, s, ch=ch: r.set_colour_input(ch)) for ch in range(4)] + [
    option("colour%d median3" % ch, U8, setup=lambda r, s, ch=ch: (r.set_colour_input(ch), r.set_frontend(3, 1, 1))) for ch in range(4)
] + [
    option("colour1 bin2x2", U8, setup=lambda r, s: (r.set_colour_input(1), r.set_frontend(0, 2, 2))),
    option("colour1 u16", U16, setup=lambda r, s: r.set_colour_input(1)),
    option("DxH", layout=capi.LAYOUT_TRANSPOSED),
    option("DxH u8 framenorm", U8, capi.LAYOUT_TRANSPOSED, cfg=dict(donotnormalize=0)),
    option("staged", setup=lambda r, s: r.set_staged(True)),
    option("staged u8", U8, setup=lambda r, s: r.set_staged(True)),
    option("plan=-2", setup=lambda r, s: r.set_plan(-2)),
    option("plan=-3", setup=lambda r, s: r.set_plan(-3)),
    option("general", setup=lambda r, s: r.set_plan(-1, True)),
    option("precise=0", setup=lambda r, s: r.set_precise_division(False)),
    option("block=64", setup=lambda r, s: r.set_launch(64, 0)),
    option("block=256", setup=lambda r, s: r.set_launch(256, 0)),
    option("grid=4", setup=lambda r, s: r.set_launch(0, 4)),
    option("A=16", cfg=dict(averages=16)),
    option("jit=0", setup=lambda r, s: r.set_jit(False)),
    option("jit=0 pi", setup=lambda r, s: (r.set_jit(False), r.set_pi_frame(np.full(s[0], 10.0)))),
]


def note(rec):
    n = rec.jit_note()
    return " | note '%s'" % n if n else ""


def line(shape, opt):
    label, dtype, layout, cfg, setup = opt
    W, M, N, D = shape
    cfg = dict(cfg)
    if cfg.pop("deep", False):
        D = N // 2 + N // 8
    head = "W=%d M=%d N=%d D=%d %s:" % (W, M, N, D, label)
    rec = None
    try:
        rec = Reconstructor(Config(width=W, height=H, numfftpoints=N, numdisplaypoints=D, increasefftpointsmultiplier=M, device=0, **cfg))
        rec.set_background(np.full(W, 1000.0))
        setup(rec, shape)
        fam = rec.prepare(dtype, layout)
        return "%s %s%s" % (head, FAMILY[fam], note(rec))
    except capi.FdoctError as e:
        err = str(e).split(": ", 1)[1]
        return "%s rc=%d '%s'%s" % (head, e.code, err, note(rec) if rec is not None and rec.h else "")
    finally:
        if rec is not None:
            rec.close()


def main():
    for shape in SHAPES:
        for opt in OPTIONS:
            if shape in FULL or opt[0] in CORE:
                print(line(shape, opt), flush=True)
    for shape in BIN_EDGES:
        for opt in OPTIONS:
            if opt[0] in ("bin2x2", "bin2x2 u8"):
                print(line(shape, opt), flush=True)


if __name__ == "__main__":
    main()
