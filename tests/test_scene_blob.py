"""CPU: what pt_scene_host.cpp makes of a description, pinned word for word.  Every case of tests/scene_blob_cases.py is created by the host emulation
(the engine's own pt_scene_host.cpp) and its blob and texel words are compared, by count and SHA-256, with tests/golden/scene_blobs.tsv; every refusal case
must be refused with the message in tests/golden/scene_refusals.tsv.  A change that means to move the blob records the fixtures again
(tools/scene_blob_digests.py); a refactor leaves them alone.
(The product library, whose pt_scene_host.cpp another compiler builds, is not held to these words: DESIGN.md section 18.)"""
import os

import pytest

import scene_blob_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def loaded():
    return cases.load()


def test_creation_cases_make_the_recorded_words(loaded):
    emu, raw = loaded
    recorded = cases.read_tsv(os.path.join(GOLDEN, "scene_blobs.tsv"))
    made = []
    for name, make in cases.creation_cases():
        scene = emu.create_scene(make())
        made.append(cases.digest_row(name, cases.scene_words(raw, scene, 0), cases.scene_words(raw, scene, 1)))
        scene.close()
    assert [r[0] for r in made] == [r[0] for r in recorded], "the case list and the fixture name different cases"
    wrong = [m[0] for m, r in zip(made, recorded) if m != r]
    assert not wrong, "blob or texel words differ from the recorded ones: %s" % ", ".join(wrong)


def test_refusal_cases_are_refused_with_the_recorded_messages(loaded):
    emu, _ = loaded
    recorded = cases.read_tsv(os.path.join(GOLDEN, "scene_refusals.tsv"))
    got = [(name, cases.refusal_message(emu, make())) for name, make in cases.refusal_cases()]
    assert got == recorded


def test_recorded_refusals_are_all_different():
    """One case per refusal site: no two cases stop at the same one."""
    messages = [m for _, m in cases.read_tsv(os.path.join(GOLDEN, "scene_refusals.tsv"))]
    assert len(set(messages)) == len(messages)


def test_the_case_without_curve_tables_takes_the_second_build(loaded, pkg):
    """Its blob fits PT_BLOB_LDS_ALL_BYTES and no curve names a cell table, while fewer of the same curves leave a smaller scene its tables: the first build, with
    the tables, was above the limit and was dropped."""
    emu, raw = loaded
    scene = emu.create_scene(cases.cornell_without_curve_tables())
    blob = cases.scene_words(raw, scene, 0)
    assert blob.size * 4 <= cases.LDS_ALL_BYTES and cases.curve_tables_dropped(blob)
    plain = emu.create_scene(pkg.scene.cornell_box())
    assert not cases.curve_tables_dropped(cases.scene_words(raw, plain, 0))


def test_the_two_certified_instances_merge_their_face_flags(loaded):
    """Both cubes are certified outward, one of them inward too; the mesh's faces keep the weaker claim: none inward."""
    emu, raw = loaded
    scene = emu.create_scene(cases.two_certified_instances())
    blob = cases.scene_words(raw, scene, 0)
    INST_OFF, INST_WORDS, INST_FLAGS, OUT, IN = 4, 40, 1, 16, 32   # pt_blob.h PT_HDR_INSTANCE_OFF, PT_INST_WORDS, PT_INST_FLAGS, PT_INST_CONVEX_OUT / _IN
    flags = [int(blob[blob[INST_OFF] + i * INST_WORDS + INST_FLAGS]) for i in (2, 3)]
    assert [bool(f & OUT) for f in flags] == [True, True] and sorted(bool(f & IN) for f in flags) == [False, True]
    assert emu._debug_scene_info(scene.handle, 16) == 0 and emu._debug_scene_info(scene.handle, 17) == 0
