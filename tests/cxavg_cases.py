"""The cases of the coherent-averaging stage's tests (tests/test_cxavg_cases.py on the CPU, tests/test_gpu_cxavg.py on the GPU), and
the launch arithmetic of the stage (fdoct_cxavg_kernels.h) restated next to them, as pure functions.

The fields are tests/angio_cases.py's: fully developed speckle that is the same in every repeat (static), drawn anew in every
repeat (independent) or half and half (vessel), a noise floor of a few counts, optionally a frame or one A-scan of one frame that
is exactly 0, and a bulk phase per (frame, A-scan) that every depth shares -- what the alignment exists to take out."""
import functools

import numpy as np

import angio_cases as ac
import cxavg_model as cm

PI = np.pi


def _case(what, frames, N, H, D, seed, stride=None, ref=0, align=1, align_range=(0, 0), **fld):
    """frames: (groups, repeats) of angio_cases.field -- groups x repeats frames, the speckle shared within a field group."""
    return dict(what=what, frames=frames, repeats=N, H=H, D=D, seed=seed, stride=stride, ref=ref, align=align, align_range=align_range, fld=fld)


CASES = [
    # the alignment modes on a static field whose frames and A-scans each carry a phase of their own
    _case("static, bulk phase, N 4, 2 groups of 5 x 257, align 1", (2, 4), 4, 5, 257, 1, bulk_phase=PI),
    _case("static, bulk phase, N 4, 2 groups of 5 x 257, align 0", (2, 4), 4, 5, 257, 1, align=0, bulk_phase=PI),
    _case("static, bulk phase, N 4, 2 groups of 5 x 257, align 2, ref 3", (2, 4), 4, 5, 257, 1, align=2, ref=3, bulk_phase=PI),
    # the kinds of speckle, ref in the middle
    _case("independent, N 4, 3 x 513, align 1, ref 2", (1, 4), 4, 3, 513, 2, ref=2, kind="independent", bulk_phase=PI),
    _case("vessel, N 3, 2 groups of 3 x 513, align 2, ref 1", (2, 3), 3, 3, 513, 3, ref=1, align=2, kind="vessel", bulk_phase=PI),
    # on each side of the boundary between the forms: 8 repeats of 2 pairs a thread are the 16 a thread keeps, 8 of 3 are streamed;
    # likewise 2 repeats of 8 pairs a thread, and 3 repeats (held as 4) of 4
    _case("vessel, N 8, 2 x 512, align 1 (register, at the boundary)", (1, 8), 8, 2, 512, 4, ref=7, kind="vessel", bulk_phase=PI),
    _case("vessel, N 8, 2 x 513, align 1 (streaming, past the boundary)", (1, 8), 8, 2, 513, 4, ref=7, kind="vessel", bulk_phase=PI),
    _case("independent, N 2, 2 x 2048, align 2 (register, at the boundary)", (1, 2), 2, 2, 2048, 5, align=2, kind="independent", bulk_phase=PI),
    _case("static, N 3, 1 x 1024, align 1, ref 1 (register, at the boundary)", (1, 3), 3, 1, 1024, 20, ref=1, bulk_phase=PI),
    _case("independent, N 2, 2 x 2049, align 2 (streaming)", (1, 2), 2, 2, 2049, 5, align=2, kind="independent", bulk_phase=PI),
    _case("independent, N 5, 2 x 1025, align 0 (streaming)", (1, 5), 5, 2, 1025, 6, align=0, kind="independent"),
    _case("static, N 5, 2 x 1025, align 1, a range that ends at the last depth (streaming)", (1, 5), 5, 2, 1025, 6, ref=4, align_range=(1000, 25),
          bulk_phase=PI),
    # the repeats' extremes
    _case("static, bulk phase, N 64, 2 x 70, align 1, ref 63 (streaming)", (1, 64), 64, 2, 70, 7, ref=63, bulk_phase=PI),
    _case("independent, N 64, 2 x 64, align 2, ref 31 (streaming)", (1, 64), 64, 2, 64, 8, ref=31, align=2, kind="independent", bulk_phase=PI),
    _case("independent, N 12, 2 x 200, align 1, ref 5 (register, held as 16 repeats)", (1, 12), 12, 2, 200, 21, ref=5, kind="independent", bulk_phase=PI),
    _case("vessel, N 2, 3 groups of 1 x 255, align 1, half the depths", (3, 2), 2, 1, 255, 9, ref=1, align_range=(0, 128), kind="vessel", bulk_phase=PI),
    # a thread's pair count and its tail; one A-scan; one depth
    _case("static, N 3, 1 x 256, align 1, a range that ends at the last depth", (1, 3), 3, 1, 256, 10, align_range=(200, 56), bulk_phase=PI),
    _case("static, N 5, 3 x 257, align 1, a range of one depth", (1, 5), 5, 3, 257, 11, ref=2, align_range=(256, 1), bulk_phase=PI),
    _case("static, N 5, 3 x 257, align 2, a range of one depth", (1, 5), 5, 3, 257, 11, ref=2, align=2, align_range=(100, 1), bulk_phase=PI),
    _case("independent, N 3, 1 x 1, align 1", (1, 3), 3, 1, 1, 12, kind="independent"),
    _case("independent, N 3, 2 groups of 1 x 1, align 2", (2, 3), 3, 1, 1, 13, align=2, ref=2, kind="independent"),
    _case("independent, N 2, 300 x 3, align 1", (1, 2), 2, 300, 3, 14, kind="independent", bulk_phase=PI),
    _case("independent, N 2, 300 x 3, align 2", (1, 2), 2, 300, 3, 14, align=2, ref=1, kind="independent", bulk_phase=PI),
    # zeros: the ref, another repeat, one A-scan of the ref and of another repeat
    _case("the ref a frame of zeros, N 4, 3 x 130, align 1", (1, 4), 4, 3, 130, 15, ref=1, zero_frame=(0, 1), bulk_phase=PI),
    _case("the ref a frame of zeros, N 4, 2 x 1100, align 2 (streaming)", (1, 4), 4, 2, 1100, 16, ref=1, align=2, zero_frame=(0, 1), bulk_phase=PI),
    _case("a repeat a frame of zeros, N 4, 3 x 130, align 1", (1, 4), 4, 3, 130, 15, ref=1, zero_frame=(0, 2), bulk_phase=PI),
    _case("a repeat a frame of zeros, N 4, 3 x 130, align 2", (1, 4), 4, 3, 130, 15, ref=1, align=2, zero_frame=(0, 2), bulk_phase=PI),
    _case("an A-scan of the ref zeros, N 3, 2 groups of 4 x 130, align 1", (2, 3), 3, 4, 130, 17, zero_row=(1, 0, 2), bulk_phase=PI),
    _case("an A-scan of a repeat zeros, N 3, 2 groups of 4 x 130, align 2", (2, 3), 3, 4, 130, 17, align=2, zero_row=(1, 1, 2), bulk_phase=PI),
    # sliding: six frames of one static field, every frame with its own phase
    _case("sliding, N 3, stride 1, 6 frames of 4 x 130, align 1", (1, 6), 3, 4, 130, 18, stride=1, ref=1, bulk_phase=PI),
    _case("sliding, N 4, stride 2, 8 frames of 2 x 1100, align 2 (streaming)", (1, 8), 4, 2, 1100, 19, stride=2, align=2, bulk_phase=PI),
]


def index(what):
    return [c["what"] for c in CASES].index(what)


def case_field(c):
    return ac.field(c["frames"][0], c["frames"][1], c["H"], c["D"], c["seed"], **c["fld"])


def case_args(c):
    """The keywords of cxavg_model's functions, and of fdoct_amd.coherent.params."""
    return dict(repeats=c["repeats"], stride=c["stride"], ref=c["ref"], align=c["align"], align_range=c["align_range"])


def case_form(c):
    """FORM_REGISTER or FORM_STREAMING, by the restated launch arithmetic."""
    return cm.geometry(c["frames"][0] * c["frames"][1], c["repeats"], c["stride"], c["H"], c["D"], c["align"])[1]


@functools.lru_cache(maxsize=None)
def case_refs(i):
    """(X, (model, tolerances)) of CASES[i]: computed once, shared, never written to."""
    c = CASES[i]
    X = case_field(c)
    kw = case_args(c)
    refs = (cm.model(X, **kw), cm.tolerances(X, **kw))
    X.setflags(write=False)
    return X, refs


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
def resident(cus):
    """resident_blocks(CUs, 16 waves per CU, 256): the cap of the stage's grid."""
    return cus * cm.BLOCKS_PER_CU


def placement_items(cus):
    """(group, A-scan) items for one and a half passes of the capped grid and a partial one."""
    return ac.placement_groups(cus)
