"""The catalogue of tests/stream_cases.py against the binding, on the CPU: every public `*_device` or `set_*` method of
fdoct_amd.capi.Reconstructor is an entry, a setter or exempt with a reason -- a new entry point fails here until the stream-order
tests know it; every growth pair's second call needs strictly more bytes of its workspace than the first; and
tests/test_gpu_stream_order.py has a case for every name.  Likewise the add-on stages: every module-level `*_device` function of the
fdoct_amd package is an ADDON_ENTRIES name or exempt; their growth pairs need strictly more bytes, by sizes that equal what the
stages' handle-free `*_plan` entry points report; each TABLE_PAIRS pair keeps its tables' sizes and moves the model's main output by
at least FAR; and tests/test_gpu_stream_order_stages.py has a case for every name."""
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


# ---- the add-on stages: module-level functions over a Reconstructor ----------------------------------------------------------------------
def test_every_module_level_device_function_is_an_addon_entry_or_exempt():
    found = sc.addon_functions()
    known = set(sc.ADDON_ENTRIES) | set(sc.ADDON_EXEMPT)
    missing = [n for n in found if n not in known]
    assert not missing, "module-level *_device functions the stream-order catalogue does not know (tests/stream_cases.py): %s" % missing
    assert len(found) >= 10, found                                 # the introspection finds the functions at all
    assert sorted(set(sc.ADDON_ENTRIES)) == sorted(sc.ADDON_ENTRIES) and set(sc.ADDON_ENTRIES) <= set(found)
    assert not (set(sc.ADDON_EXEMPT) & set(sc.ADDON_ENTRIES)) and set(sc.ADDON_EXEMPT) <= set(found)
    assert all(isinstance(why, str) and len(why) > 20 and "\n" not in why for why in sc.ADDON_EXEMPT.values())


def test_addon_growth_pairs_need_strictly_more_bytes():
    assert len(set(sc.ADDON_GROWTH_IDS)) == len(sc.ADDON_GROWTH) and not (set(sc.ADDON_GROWTH_IDS) & set(sc.GROWTH_IDS))
    for g in sc.ADDON_GROWTH:
        small, large = g.need(g, g.small), g.need(g, g.large)
        assert 0 < small < large, (g.workspace, small, large)
        assert set(g.small) == set(g.large) and len(g.small) == 1, g.workspace
        stage, shape, p, want = g.call
        assert list(g.small)[0] in shape or list(g.small)[0] in p, g.workspace        # the key names something the call has
    assert not (set(sc.GROWTH_EXEMPT) & set(sc.ADDON_GROWTH_IDS))
    for name in ("ws_disp_tab", "ws_vib_ref", "ws_vib_tab", "ws_vib_part", "ws_ang_bulk", "ws_cxa", "ws_ssa", "ws_ssa_tab", "stage_out (scratch)"):
        assert name in sc.ADDON_GROWTH_IDS, name


def test_addon_restated_sizes_at_known_points():
    """The add-on workspaces' restated sizes at shapes worked out by hand from the sites they name."""
    ssa = dict(groups=1, repeats=2, ascans=3, n=60)
    assert sc.ssada_bytes(ssa, dict(repeats=2, bands=2))["ws_ssa_tab"] == 60 * 8 + 2 * 60 * 4 == 960
    assert sc.ssada_bytes(ssa, dict(repeats=2, bands=5))["ws_ssa_tab"] == 1680
    assert sc.ssada_bytes(ssa, dict(repeats=2, bands=3))["ws_ssa"] == 3 * 3 * 30 * (8 * 2 + 8) == 6480       # default depths: dc 30
    assert sc.ssada_bytes(dict(ssa, groups=3), dict(repeats=2, bands=3, max_workspace_bytes=6480))["ws_ssa"] == 6480   # one group a pass
    disp = dict(rows=2, n=16)
    assert sc.dispersion_bytes(disp, dict(grid=(3, 1)))["ws_disp_tab"] == (1 + 3 + 1) * 16 * 8 == 640
    assert sc.dispersion_bytes(disp, dict(grid=(5, 2)))["ws_disp_tab"] == 1024
    # cos_sin alone: sums 48 -> 256, row_sums 96 -> 256, best 40 -> 256; with 6 rows row_sums 288 -> 512
    assert sc.dispersion_bytes(disp, dict(grid=(3, 1)), ("cos_sin",))["stage_out (scratch)"] == 768
    assert sc.dispersion_bytes(dict(rows=6, n=16), dict(grid=(3, 1)), ("cos_sin",))["stage_out (scratch)"] == 1024
    assert sc.dispersion_bytes(disp, dict(grid=(3, 1)))["stage_out (scratch)"] == 0
    vib = dict(nframes=6, ascans=3, depths=5)
    b = sc.vibro_bytes(vib, dict(freq=(0.11,), ref=(0, 1)))
    assert b == {"ws_vib_ref": 6 * 3 * 8, "ws_vib_tab": (6 + 1 * 2 * 2 + 3 * 2) * 16, "ws_vib_part": 0}          # one chunk: no partials
    b = sc.vibro_bytes(dict(vib, nframes=8), dict(freq=(0.11,), chunk_steps=2))
    assert b == {"ws_vib_ref": 0, "ws_vib_tab": (8 + 4 * 2 * 2 + 3 * 2) * 16, "ws_vib_part": 4 * 7 * 15 * 8}     # 7 steps: 4 chunks of 7 sums
    assert sc.vibro_bytes(vib, dict(freq=(0.11,), ref=(0, 1)), ("rms",)) == {"ws_vib_ref": 144, "ws_vib_tab": 0, "ws_vib_part": 0}
    ang = dict(nframes=6, repeats=2, ascans=3, depths=16)
    assert sc.angio_bytes(ang, dict(repeats=2, bulk=(0, 8)))["ws_ang_bulk"] == 3 * 1 * 3 * 8 == 72
    assert sc.angio_bytes(ang, dict(repeats=2, bulk=(0, 8)), ("var", "power"))["ws_ang_bulk"] == 0 == sc.angio_bytes(ang, dict(repeats=2))["ws_ang_bulk"]
    assert sc.cxavg_bytes(ang, dict(repeats=2, align=2))["ws_cxa"] == (6 + 6 * 3) * 8 == 192
    assert sc.cxavg_bytes(ang, dict(repeats=2, align=1))["ws_cxa"] == 0


def _plans():
    """stage -> (shape, p) -> workspace_bytes of the stage's handle-free *_plan entry point."""
    from fdoct_amd import angiography, coherent, dispersion, ssada, vibrometry

    def disp(shape, p):
        a2, a3, depth = sc.disp_axes(p)
        return dispersion.plan(a2, a3, shape["rows"], shape["n"], depth)["workspace_bytes"]
    return {
        "ssada": lambda s, p: ssada.plan(dict(p, n=s["n"]), s["groups"] * s["repeats"], s["ascans"], s["n"])["workspace_bytes"],
        "dispersion": disp,
        "vibro": lambda s, p: vibrometry.plan(p, s["nframes"], s["ascans"], s["depths"])["workspace_bytes"],
        "angio": lambda s, p: angiography.plan(p, s["nframes"], s["ascans"], s["depths"])["workspace_bytes"],
        "cxavg": lambda s, p: coherent.plan(p, s["nframes"], s["ascans"], s["depths"])["workspace_bytes"],
    }


def _restated_plan_bytes(stage, shape, p):
    """What the stage's *_plan reports as workspace_bytes, from the restated sizes: fdoct_ssada_plan the pass's workspace without
    the table; fdoct_dispersion_plan the table and all four outputs; the others the sum of their workspaces (every output asked for)."""
    b = sc.STAGE_BYTES[stage](shape, p)
    if stage == "ssada":
        return b["ws_ssa"]
    if stage == "dispersion":
        return b["ws_disp_tab"] + b["outputs"]
    return sum(b.values())


def test_restated_sizes_equal_what_the_plan_entry_points_report():
    import os

    import pytest
    from fdoct_amd import capi, ssada
    if not (os.path.exists(capi.library_path()) and os.path.exists(ssada.library_path())):
        pytest.skip("the libraries are not built: the *_plan entry points cannot be asked")
    plans = _plans()
    calls = [(t.stage, t.shape, p) for t in sc.TABLE_PAIRS for p in (t.p1, t.p2)]
    for g in sc.ADDON_GROWTH:
        calls += [sc.addon_call(g, which)[:3] for which in (g.small, g.large)]
    calls.append(("ssada", dict(groups=3, repeats=2, ascans=3, n=60), dict(repeats=2, bands=3, max_workspace_bytes=6480)))
    for stage, shape, p in calls:
        assert plans[stage](shape, p) == _restated_plan_bytes(stage, shape, p), (stage, shape, p)
    assert {c[0] for c in calls} == set(sc.ADDON_STAGES)


def test_table_pairs_share_their_tables_sizes_and_differ_in_the_main_output():
    """The condition under which a reach-back through a per-call table shows: under p1 and p2 every workspace of the call has the
    same size (nothing is reserved anew, so nothing drains), and the stage's model alone puts the main output at least FAR apart."""
    assert sorted(sc.TABLE_PAIR_IDS) == sorted(sc.ADDON_STAGES)
    for t in sc.TABLE_PAIRS:
        b1, b2 = sc.STAGE_BYTES[t.stage](t.shape, t.p1), sc.STAGE_BYTES[t.stage](t.shape, t.p2)
        assert b1 == b2, (t.stage, b1, b2)
        assert t.tables and all(b1[w] > 0 for w in t.tables), (t.stage, b1)
        assert t.p1 != t.p2
        X = sc.addon_field(t.stage, t.shape, t.seed)
        a, b = sc.addon_model(t.stage, X, t.p1)[t.main], sc.addon_model(t.stage, X, t.p2)[t.main]
        assert a.shape == b.shape and np.isfinite(np.ascontiguousarray(a).view(np.float32 if a.dtype.itemsize % 8 else np.float64)).all()
        d = sc.distance(a, b)
        print("%s: model distance of %s between p1 and p2: %.3g" % (t.stage, t.main, d))
        assert d >= sc.FAR, "%s: the model's %s under p1 and under p2 are %.3g apart: a reach-back would not show" % (t.stage, t.main, d)


def test_the_stage_tests_have_a_case_for_every_addon_name():
    import test_gpu_stream_order_stages as t
    t.test_the_catalogue_has_a_case_for_every_addon_name()
    # a growth case has a handle pair to itself
    keys = [build().key for reg in (t.RESIDENCY, t.TABLES, t.ALT, t.HOST_CASES) for build in reg.values()]
    growth_keys = [t.GROWTH[g.workspace]().key for g in sc.ADDON_GROWTH]
    assert len(set(growth_keys)) == len(growth_keys) and not (set(growth_keys) & set(keys))
    for reg in (t.RESIDENCY, t.TABLES, t.ALT, t.GROWTH, t.HOST_CASES):
        for name, build in reg.items():
            case = build()
            assert case.steps and callable(case.prep) and callable(case.make), name
            for a in case.inputs.values():
                assert isinstance(a, np.ndarray) and a.size, name
