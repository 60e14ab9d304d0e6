"""The descriptions behind tests/test_scene_blob.py and tools/scene_blob_digests.py: CREATION, the scenes whose blob and texel words are pinned
(tests/golden/scene_blobs.tsv), and REFUSALS, one description per refusal of pt_scene_host.cpp's scene build that Python can reach, each valid
except for that fault and paired with its message (tests/golden/scene_refusals.tsv).  A helper module, not a test."""
import ctypes as C
import hashlib
import importlib
import inspect
import os

import numpy as np

import emulation
import fuzz_scenes

FUZZ_SEEDS = (*range(0, 40), *range(100000, 100010), *range(140000, 140020), *range(150000, 150020), *range(190000, 190010), *range(200000, 200010),
              *range(600000, 600010))   # every seed class of fuzz_scenes.random_scene
LDS_ALL_BYTES = 24576   # pt_blob.h PT_BLOB_LDS_ALL_BYTES
CURVE_RECORD = (8, 6)   # pt_blob.h PT_CURVE_WORDS, PT_CURVE_GRID
HDR_CURVE_OFF, HDR_CURVE_COUNT = 19, 20


def _pkg():
    return importlib.import_module("rust-pathtracer_amd")


# ---- creation ----------------------------------------------------------------------------------------------------------------------------
NOT_SCENES = ("cornell_obj_text", "synthetic_hdri", "transform_from_data")   # scene.py's public functions without a required argument that make something else


def named_scenes():
    """Every public function of scene.py that takes no required argument and makes a scene, by name: a new one is pinned by recording it."""
    S = _pkg().scene
    out = {}
    for name, fn in sorted(vars(S).items()):
        if name.startswith("_") or name in NOT_SCENES or not inspect.isfunction(fn) or fn.__module__ != S.__name__:
            continue
        if all(p.default is not p.empty for p in inspect.signature(fn).parameters.values()):
            out[name] = fn
    return out


def cornell_without_curve_tables():
    """cornell_box plus tabulated library curves that nothing uses: with their cell tables the blob is above PT_BLOB_LDS_ALL_BYTES, without them not above, so
    build_host_scene keeps its second build, the one without tables (curve_tables_dropped() says whether a blob is such a build).  23744 bytes without; the
    tables are 32 words for each of the six curves of 76 and 81 knots (128 cells) and 64 for each of the two of 141 (256 cells): 1280 bytes more, 25024, above 24576."""
    S = _pkg().scene
    b = S.cornell_box()
    S.add_library_curves(b, ["D65", "srgb_r", "srgb_g", "srgb_b", "copper_n", "copper_k"])
    return b


def curve_tables_dropped(blob):
    """No curve record of the blob names a cell table although a tabulated curve of 8..255 knots is there (cornell_box's own have tables when built alone)."""
    words, grid = CURVE_RECORD
    return not any(blob[blob[HDR_CURVE_OFF] + i * words + grid] for i in range(blob[HDR_CURVE_COUNT]))


def two_certified_instances():
    """Two convex-certified instances of one cube mesh with different claims: a small lamp sits inside the first cube's box, so that one is certified outward only, the
    other both ways, and the face flags in the mesh's triangle records are the merge of the two (the weaker claim per face)."""
    pkg = _pkg()
    S, api = pkg.scene, pkg.api
    b = S.SceneBuilder()
    S.add_library_curves(b, ["flat_zero"])
    b.set_environment_constant(b.curve("flat_zero"), 0.0)
    white, glass, lamp = (S.add_library_material(b, n) for n in ("lambertian_white", "ggx_glass", "diffuse_light_flat_x5"))
    b.add_rect((8, 8), (0.0, 0.0, -1.5), "Z", True, white)
    b.add_rect((1.0, 1.0), (0.0, 0.0, 3.0), "Z", True, lamp)
    p = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.float32) - 0.5
    f = np.array([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (1, 2, 6), (1, 6, 5), (2, 3, 7), (2, 7, 6), (3, 0, 4), (3, 4, 7)], np.uint32)
    cube = b.add_mesh(p, f, None, face_materials=api.material_id(api.TAG_MATERIAL, white & 0xFFFF))
    b.add_mesh_instance(cube, glass, S.transform_from_data((0.8, 0.8, 0.8), None, (-0.9, 0.0, 0.0)))
    b.add_mesh_instance(cube, glass, S.transform_from_data((0.6, 0.9, 0.7), [((0.0, 0.0, 1.0), 30.0)], (0.9, 0.0, 0.0)))
    b.add_sphere(0.05, (-0.9, 0.0, 0.0), lamp)
    b.add_camera((4.0, 0.5, 1.0), (0.0, 0.0, -0.3), 40.0, focal_distance=4.0, aperture_diameter=0.0)
    return b


def creation_cases():
    """[(name, function that makes the description)]"""
    cases = list(named_scenes().items())
    cases += [("fuzz_%d" % seed, (lambda seed=seed: fuzz_scenes.random_scene(seed))) for seed in FUZZ_SEEDS]
    cases += [("cornell_without_curve_tables", cornell_without_curve_tables), ("two_certified_instances", two_certified_instances)]
    return cases


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
class Edited:
    """A description with one field changed after it was flattened (the arrays of a flattened description are copies: the builder stays whole)."""

    def __init__(self, builder, edit):
        self.builder, self.edit = builder, edit

    def desc(self):
        d, keep = self.builder.desc()
        self.edit(d)
        return d, keep


def _base(hdr=False, mediums=2):
    """One of everything the build checks.  Materials: 0 error light, 1 lambertian, 2 ggx, 3 diffuse light, 4 passthrough; mediums: 0 HG, 1 Rayleigh (and more HG);
    mesh 0, an octahedron with vertex normals and face materials; instances: 0 the mesh, 1 rect, 2 sphere, 3 disk; texstack 0 = layer 0, one texel."""
    pkg = _pkg()
    S, api = pkg.scene, pkg.api
    b = S.SceneBuilder()
    S.add_library_curves(b, ["flat_one", "flat_zero", "E5", "cornell_white", "srgb_r", "srgb_g", "srgb_b"])
    one, zero = b.curve("flat_one"), b.curve("flat_zero")
    lam = b.material_lambertian("lam", b.texstack_texture1("white", b.curve("cornell_white")))
    ggx = b.material_ggx("ggx", 0.1, b.curve_cauchy(None, 1.45, 3540.0), one, zero)
    light = b.material_diffuse_light("light", b.curve("E5"), zero, api.SIDED_DUAL)
    hg = b.medium_hg("hg", zero, zero, one)
    b.medium_rayleigh("rayleigh", b.curve_cauchy(None, 1.3, 2000.0), 1.0)
    for k in range(mediums - 2):
        b.medium_hg("hg%d" % k, zero, zero, one)
    passthrough = b.material_passthrough("pass", one, 0, hg)
    p, f, n = S._octahedron()
    b.add_mesh_instance(b.add_mesh(p, f, n, face_materials=lam), None)
    b.add_rect((1.0, 1.0), (0.0, 0.0, 2.0), "Z", True, light)
    b.add_sphere(0.3, (1.5, 0.0, 0.0), ggx)
    b.add_disk(0.3, (-1.5, 0.0, 0.0), True, passthrough)
    b.add_camera((4.0, 0.0, 1.0), (0.0, 0.0, 0.0), 40.0)
    if hdr:
        sky = b.texstack_texture4("sky", [b.curve(c) for c in ("srgb_r", "srgb_g", "srgb_b", "flat_zero")], S.synthetic_hdri(8, 4))
        b.set_environment_hdr(sky, 1.0, importance=(4, 4))
    else:
        b.set_environment_constant(one, 0.5)
    return b


def _set(path, value):
    """An edit: `path` is an attribute path from the description, e.g. "materials[2].alpha"."""
    def edit(d):
        exec("d.%s = value" % path, {"d": d, "value": value})
    return edit


def _both(*edits):
    def edit(d):
        for e in edits:
            e(d)
    return edit


def refusal_cases():
    """[(name, function that makes the description)]: the name is the fault; the message is the fixture's."""
    api = _pkg().api
    beyond = api.material_id(api.TAG_MATERIAL, 999)
    plain = [
        ("no_materials", _set("material_count", 0)),
        ("no_camera", _set("camera_count", 0)),
        ("environment_kind", _set("environment.kind", 7)),
        ("environment_curve", _set("environment.curve", -1)),
        ("curve_kind", _set("curves[0].kind", 99)),
        ("curve_data_range", _set("curves[0].data_count", 10 ** 6)),
        ("curve_table_empty", _set("curves[1].data_count", 0)),
        ("lambertian_texstack", _set("materials[1].texstack", 9)),
        ("ggx_curve", _set("materials[2].curve_kappa", 999)),
        ("ggx_alpha", _set("materials[2].alpha", 0.0)),
        ("light_curve", _set("materials[3].curve_emit", -1)),
        ("passthrough_curve", _set("materials[4].curve_bounce", 999)),
        ("material_kind", _set("materials[1].kind", 99)),
        ("material_medium", _set("materials[2].inner_medium", 9)),
        ("mediums_missing", _set("mediums", C.POINTER(api.Medium)())),
        ("hg_curve", _set("mediums[0].curve_g", 999)),
        ("rayleigh_curve", _set("mediums[1].curve_ior", -1)),
        ("medium_kind", _set("mediums[0].kind", 9)),
        ("texstack_layers", _set("texstacks[0].layer_count", 5)),
        ("layer_kind", _set("layers[0].kind", 9)),
        ("texture_empty", _set("layers[0].width", 0)),
        ("texture_data_range", _set("layers[0].data_offset", 10 ** 6)),
        ("texture_curve", _set("layers[0].curves[0]", 999)),
        # (a texture beyond 2^32 texels, described and never read: the build refuses before it looks at a texel)
        ("texture_too_large", _both(_set("texture_data_count", 2 ** 33), _set("layers[0].data_offset", 2 ** 32))),
        ("mesh_vertices", _set("meshes[0].vertex_count", 10 ** 6)),
        ("mesh_indices", _set("meshes[0].face_count", 10 ** 6)),
        ("mesh_normals", _set("meshes[0].normal_offset", 10 ** 6)),
        ("mesh_face_materials", _set("meshes[0].face_material_offset", 10 ** 6)),
        ("mesh_no_faces", _set("meshes[0].face_count", 0)),
        ("mesh_index", _set("indices[0]", 99)),
        ("mesh_face_material", _set("face_materials[0]", beyond)),
        ("instance_material", _set("instances[2].material", beyond)),
        ("rect_size", _set("instances[1].size[0]", 0.0)),
        ("sphere_radius", _set("instances[2].radius", 0.0)),
        ("disk_radius", _set("instances[3].radius", 0.0)),
        ("instance_mesh", _set("instances[0].mesh", 5)),
        ("shape_kind", _set("instances[2].kind", 9)),
    ]
    hdr = [
        ("environment_texstack", _set("environment.texstack", 99)),
        ("importance_size", _set("environment.importance_width", 20000)),
        ("importance_luminance_curve", _set("environment.importance_luminance_curve", 999)),
    ]
    cases = [(name, (lambda edit=edit: Edited(_base(), edit))) for name, edit in plain]
    cases += [(name, (lambda edit=edit: Edited(_base(hdr=True), edit))) for name, edit in hdr]
    cases.append(("too_many_mediums", lambda: _base(mediums=256)))
    return cases


# ---- what is compared --------------------------------------------------------------------------------------------------------------------
_SWITCHES = ("PTEMU_FLAGS", "PTEMU_NO_CONVEX", "PTEMU_NO_MESH_SHORTCUTS")   # (ptemu_scene_create edits the blob under them)


def load():
    """The emulation library, and its word export bound with plain ctypes."""
    assert not any(s in os.environ for s in _SWITCHES), "the pinned blobs are those of a plain environment"
    emu = emulation.load(_pkg(), "ptemu")
    raw = C.CDLL(emulation.library_path("ptemu"))
    raw.ptemu_debug_scene_words.restype = C.c_size_t
    raw.ptemu_debug_scene_words.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    return emu, raw


def scene_words(raw, scene, which):
    """The words of a created scene: which = 0 the blob, 1 the texels and importance-map tables."""
    n = raw.ptemu_debug_scene_words(scene.handle, which, None, 0)
    out = np.zeros(n, np.uint32)
    assert raw.ptemu_debug_scene_words(scene.handle, which, out.ctypes.data, n) == n
    return out


def refusal_message(emu, description):
    api = _pkg().api
    try:
        emu.create_scene(description).close()
    except api.PtError as e:
        assert e.status == api.PT_ERR_INVALID_ARGUMENT
        return emu.last_error()
    raise AssertionError("the description was accepted")


def digest_row(name, blob, tex):
    return (name, str(blob.size), hashlib.sha256(blob.tobytes()).hexdigest(), str(tex.size), hashlib.sha256(tex.tobytes()).hexdigest())


def read_tsv(path):
    with open(path) as f:
        return [tuple(line.rstrip("\n").split("\t")) for line in f if line.strip()]
