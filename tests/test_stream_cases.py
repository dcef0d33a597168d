"""The catalogue of tests/stream_cases.py against the binding, on the CPU: every public `*_device` or `set_*` method of
fdoct_amd.capi.Reconstructor is an entry, a setter or exempt with a reason -- a new entry point fails here until the stream-order
tests know it; every growth pair's second call needs strictly more bytes of its workspace than the first; and
tests/test_gpu_stream_order.py has a case for every name."""
import numpy as np

import stream_cases as sc
from fdoct_amd.capi import Reconstructor


def test_every_device_and_set_method_is_listed_or_exempt():
    known = set(sc.ENTRIES) | set(sc.SETTERS) | set(sc.EXEMPT)
    missing = [n for n in sc.must_be_listed(Reconstructor) if n not in known]
    assert not missing, "Reconstructor methods the stream-order catalogue does not know (tests/stream_cases.py): %s" % missing
    assert len(sc.must_be_listed(Reconstructor)) >= 35          # the introspection finds the methods at all


def test_the_catalogue_names_methods_that_exist():
    methods = set(sc.public_methods(Reconstructor))
    for name in list(sc.ENTRIES) + list(sc.SETTERS) + list(sc.EXEMPT) + list(sc.DRAINING_ENTRIES):
        assert name in methods, name
    assert len(set(sc.ENTRIES)) == len(sc.ENTRIES) and len(set(sc.SETTERS)) == len(sc.SETTERS)
    assert not (set(sc.EXEMPT) & (set(sc.ENTRIES) | set(sc.SETTERS)))
    assert all(isinstance(why, str) and len(why) > 20 and "\n" not in why for why in sc.EXEMPT.values())
    assert set(sc.DRAINING_ENTRIES) <= set(sc.ENTRIES) and set(sc.TABLE_SETTERS) <= set(sc.SETTERS)


def test_every_device_method_is_an_entry_and_every_set_method_a_setter_or_an_entry():
    for n in sc.must_be_listed(Reconstructor):
        if n in sc.EXEMPT:
            continue
        if n.endswith("_device"):
            assert n in sc.ENTRIES, n
        else:
            assert n in sc.SETTERS or n in sc.ENTRIES, n


def test_growth_pairs_need_strictly_more_bytes():
    assert len(set(sc.GROWTH_IDS)) == len(sc.GROWTH)
    for g in sc.GROWTH:
        small, large = g.need(g.small), g.need(g.large)
        assert 0 < small < large, (g.workspace, small, large)
        assert set(g.small) == set(g.large) and len(g.small) == 1, g.workspace
    assert not (set(sc.GROWTH_EXEMPT) & set(sc.GROWTH_IDS))


def test_restated_sizes_at_known_points():
    """The restated reserve sizes at shapes worked out by hand from the sites they name."""
    G = {g.workspace: g for g in sc.GROWTH}
    assert G["ws_ylin"].need(dict(nframes=1)) == 11 * 1024 * 8               # 11 rows of N / 2 = 1024 float2
    assert G["ws_cx"].need(dict(nframes=2)) == 2 * 11 * 1001 * 8
    assert G["ws_tr"].need(dict(nframes=1)) == 2 * 11 * 1001 * 4
    assert G["d_minmax"].need(dict(nframes=2)) == (2 + 32) * 8
    assert G["ws_dop_bulk"].need(dict(nframes=3)) == 3 * 7 * 8
    assert G["ws_sim"].need(dict(nframes=4)) == 2 * 11 * 2048 * 2
    assert G["ws_front"].need(dict(nframes=1)) == 11 * 4096 == G["ws_med"].need(dict(nframes=1))
    assert G["ws_lp_bins"].need(dict(rows=2)) == 2 * 4 * 585 * 8
    assert G["ws_cal_mm"].need(dict(rows=8)) == 4 * 8 * 8
    assert G["d_sf_part"].need(dict(nframes=3)) == 3 * 16 == G["d_disp_part"].need(dict(nbscans=3))
    assert G["ws_col_sum"].need(dict(nframes=1)) == 8 * 64 * 8
    assert G["ws_big_*"].need(dict(nframes=2)) == 2 * 11 * 2048 * 4
    assert G["ws_mov"].need(dict(nframes=1)) == 11 * 2048 * 4 == G["ws_f32 + ws_f32_lo"].need(dict(nframes=1)) - 32


def test_the_gpu_tests_have_a_case_for_every_name():
    import test_gpu_stream_order as t
    t.test_the_catalogue_has_a_case_for_every_name()
    for name, (fam, kind) in sc.TABLE_SETS.items():
        for setter in sc.TABLE_SETTERS:
            cases = [n for n in t.SETTERS if n.startswith(setter + " ") or n.startswith(setter + " [")]
            on_set = [n for n in cases if n.endswith(" on " + name)]
            assert on_set, (setter, name)
    # a growth case has a handle pair to itself: what its workspace held before call B is call A's need, and no more
    keys = [build().key for reg in (t.RESIDENCY, t.SETTERS) for build in reg.values()]
    growth_keys = [t.GROWTH[g.workspace]().key for g in sc.GROWTH]
    assert len(set(growth_keys)) == len(growth_keys) and not (set(growth_keys) & set(keys))
    # every case can be built without a GPU, and its inputs are what its calls name
    for reg in (t.RESIDENCY, t.SETTERS, t.GROWTH):
        for name, build in reg.items():
            case = build()
            assert case.steps and callable(case.prep) and callable(case.make), name
            for a in case.inputs.values():
                assert isinstance(a, np.ndarray) and a.size, name
