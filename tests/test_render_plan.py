"""Which kernel forms a render takes, pinned.  CPU: pt_plan.cpp's plan_scene and plan_render, through the host emulation's exports, over every scene, render kind
and tuning of tests/render_plan_cases.py must give tests/golden/render_plans.tsv line for line, and the full rows its lines stand for; the table must reach every form and both values of every switch;
the one refusal is refused.  A change that means to move a choice records the table again (tools/render_plan_table.py) and its diff is the review; a refactor leaves
it alone.  GPU: the engine's scene facts are the host function's, and a render's profile shows what the host plan predicts."""
import os
import re

import pytest

import render_plan_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_plans.tsv")


@pytest.fixture(scope="module")
def loaded():
    return cases.load()


def _recorded():
    with open(GOLDEN) as f:
        return [line.rstrip("\n") for line in f if line.strip()]


def _literal(lines):
    """(the full rows the literal lines of a table stand for, its digest lines)"""
    body = [line for line in lines if not line.startswith("#")]
    return cases.expand([line for line in body if line.split("\t")[1] != "sha256"]), [line for line in body if line.split("\t")[1] == "sha256"]


def test_the_plans_are_the_recorded_ones(loaded):
    full = []
    made, recorded = cases.table(*loaded, full=full), _recorded()
    assert sorted(_literal(made)[0]) == sorted(full), "the table's lines do not stand for the rows they were made from"
    rows, digests = _literal(recorded)
    assert len(rows) == len(full) and [d.split("\t")[0] for d in digests] == ["fuzz_%d" % s for s in cases.FUZZ_SEEDS], "the case list and the fixture name different cases"
    wrong = sorted(set(full) ^ set(rows))
    assert not wrong, "%d plans differ from the recorded ones, the first: %s" % (len(wrong) // 2, ", ".join("%s %s %s" % r[:3] for r in wrong[:8]))
    assert made == recorded


def test_the_table_reaches_every_form_and_both_values_of_every_switch():
    full, digests = _literal(_recorded())
    rows = [dict(zip(cases.COLUMNS, r)) for r in full]
    assert len(rows) == len([s for s in cases.scenes() if s[2]]) * len(cases.render_kinds()) * len(cases.tunings()) and len(digests) == len(cases.FUZZ_SEEDS)

    def seen(column):
        return {r[column] for r in rows}
    assert seen("trav_form") == {"ANY", "WALK", "SWEEP", "PARKED", "PARKED_WALK"}   # (POOLED: a measurement build's, never the product's)
    assert seen("shade_form") == set(cases.SHADE_FORMS)
    for switch in ("fuse", "park_dynamic", "park_big", "live_list", "camera_record", "overlap"):
        assert seen(switch) == {"0", "1"}, switch
    assert seen("lds_mode") == set(cases.LDS_MODES)
    lacks = {int(v) for v in seen("lacks")}
    for bit in (1, 2):   # pt_device.h PT_SCENE_NO_XF, PT_SCENE_NO_LIGHTS
        assert {bool(v & bit) for v in lacks} == {False, True}, bit
    # where the issue of this table expected them
    assert {r["trav_form"] for r in rows if r["tuning"] == "NO_SWEEP"} >= {"PARKED_WALK"} and {r["trav_form"] for r in rows if r["tuning"] == "NO_SWEEP|NO_PARK"} >= {"WALK"}
    assert "1" in {r["park_big"] for r in rows if r["scene"] == "cornell_gem"}


def test_blocks_per_cu_out_of_range_is_refused(loaded, pkg):
    emu, raw = loaded
    scene = emu.create_scene(pkg.scene.cornell_box())
    rd = cases.render_kinds()[1][1]
    assert isinstance(cases.plan_render(raw, scene, cases.tuning(blocks_per_cu=1024), rd), dict)
    assert cases.plan_render(raw, scene, cases.tuning(blocks_per_cu=1025), rd) == pkg.api.PT_ERR_INVALID_ARGUMENT
    assert emu.last_error() == "pt_tuning::blocks_per_cu (PT_AMD_BLOCKS_PER_CU) must be in 1..1024"


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
HDR_FLAGS = 21   # pt_blob.h PT_HDR_FLAGS


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", ["default", "NO_LDS"])
@pytest.mark.parametrize("name", ["cornell_box", "cornell_gem", "hdri_small"])
def test_the_engine_scene_facts_are_the_host_functions(loaded, engine, pkg, name, tuning):
    """Scene creation only: the blob's flag word, lacks and the staging mode of the engine's scene against plan_scene over the emulation's copy of the scene."""
    emu, raw = loaded
    tn = dict(cases.tunings())[tuning]
    builder = getattr(pkg.scene, name)()
    want = cases.plan_scene(raw, emu.create_scene(builder), tn)
    scene = engine.create_scene(builder, tn)
    info = engine._debug_scene_info
    got = {"flags": info(scene.handle, 1000000 + HDR_FLAGS), "lacks": info(scene.handle, 9), "lds_mode": info(scene.handle, 1)}
    scene.close()
    assert got == want


# name: (scene, tuning, render kind of cases.render_kinds, what the host plan must say of it)
PROFILE_CASES = {
    "parked": ("cornell_gem", "NO_CONVEX", "plain_ls2", dict(trav_form="PARKED", park_big=1, launch_park_block=512)),
    "parked_walk": ("cornell_gem", "NO_SWEEP", "plain_ls2", dict(trav_form="PARKED_WALK")),
    "sweep_fused": ("cornell_box", "default", "plain_ls0", dict(trav_form="SWEEP", fuse=1)),
    "any": ("cornell_gem", "NO_PARK", "plain_ls2", dict(trav_form="ANY", fuse=0)),
    "medium": ("cornell_box", "default", "medium_aware", dict(shade_form="MEDIUM")),
    "routed": ("cornell_box", "default", "routed", dict(trav_form="ANY", shade_form="FULL")),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PROFILE_CASES))
def test_the_profile_shows_what_the_host_plan_predicts(loaded, engine, pkg, case):
    """32 x 24, 10 spp, one pass: the plan computed on the host with the engine's CU count against the profile of the render it describes."""
    emu, raw = loaded
    name, tuning, kind, expected = PROFILE_CASES[case]
    tn = dict(cases.tunings())[tuning]
    _, rd, _, routed = next(k for k in cases.render_kinds() if k[0] == kind)
    rd.width, rd.height = 32, 24
    num_cus = int(re.search(r"(\d+) CUs", engine.device_info()).group(1))
    builder = getattr(pkg.scene, name)()
    plan = cases.plan_render(raw, emu.create_scene(builder), tn, rd, None, routed, num_cus)
    named = {"trav_form": cases.TRAV_FORMS, "shade_form": cases.SHADE_FORMS}
    assert {k: (named[k][plan[k]] if k in named else plan[k]) for k in expected} == expected, "the case is not the one its name says"
    scene = engine.create_scene(builder, tn)
    prof = (scene.render_path_passes(rd, read_passes=False) if routed else scene.render(rd))[-1]
    scene.close()
    assert prof.kernel_launches[0] == 1   # (one pass)
    assert (prof.kernel_launches[1] == 0) == bool(plan["fuse"])
    assert prof.stage_items[6] == plan["launch_park_block"]
    assert prof.stage_items[7] == plan["camera_record"]
    assert (prof.kernel_launches[3] > 0) == (rd.light_samples > 0)
