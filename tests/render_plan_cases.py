"""The inputs behind tests/test_render_plan.py and tools/render_plan_table.py: which scenes, render kinds and tunings the table of the engine's form choice
(tests/golden/render_plans.tsv) is made over, and how a row is computed — by pt_plan.cpp's plan_scene and plan_render, which the host emulation exports as
ptemu_plan_scene and ptemu_plan_render (plain ctypes, as ptemu_debug_scene_words is).  A helper module, not a test."""
import ctypes as C
import hashlib
import importlib

import emulation
import fuzz_scenes
import scene_blob_cases

NUM_CUS, WIDTH, HEIGHT = 256, 64, 48
FUZZ_SEEDS = (0, 100000, 140000, 150000, 190000, 200000, 600000)   # one seed of each seed class of scene_blob_cases.FUZZ_SEEDS
TRAV_FORMS = ("ANY", "WALK", "SWEEP", "POOLED", "PARKED", "PARKED_WALK")   # pt_forms.h PT_FORM_*
SHADE_FORMS = ("LEAN", "NO_ENV", "FULL", "MEDIUM")                          # PT_SHADE_*
LDS_MODES = ("NONE", "ALL", "CORE")                                         # PT_LDS_*
# ptemu_plan_render's words: pth::RenderPlan's fields in the order of their declaration, then plan_scene's lacks and lds_mode
FIELDS = ("capacity", "grid", "hero", "park_block", "park_block_extend", "trav_form", "shade_form", "park_dynamic", "park_big", "live_list", "camera_record",
          "path_fields", "item_fields", "lds_bytes", "dyn_grid", "walk_policy", "launch_park_block", "launch_park_block_extend", "park_blob_bytes", "certs",
          "mesh_lights", "fuse", "overlap", "lacks", "lds_mode")
COLUMNS = ("scene", "kind", "tuning", "flags") + FIELDS   # flags: the blob's flag word as plan_scene leaves it
_NAMED = {"trav_form": TRAV_FORMS, "shade_form": SHADE_FORMS, "lds_mode": LDS_MODES}
_HEX = ("flags", "walk_policy")


def _api():
    return importlib.import_module("rust-pathtracer_amd").api


def tuning(**fields):
    """The default tuning (park_dynamic -1: by staging mode) with `fields` changed."""
    return _api().Tuning(**{"park_dynamic": -1, **fields})


def tunings():
    """[(name, Tuning)]"""
    api = _api()
    flags = ("NO_LDS", "NO_CORE_LDS", "NO_PARK", "NO_SWEEP", "NO_SWEEP|NO_PARK", "GENERAL_FORMS", "NO_FUSE", "NO_LIVE_LIST", "NO_CONVEX", "NO_PASS_OVERLAP")
    out = [("default", tuning())]
    for name in flags:
        bits = 0
        for part in name.split("|"):
            bits |= getattr(api, "TUNE_" + part)
        out.append((name, tuning(flags=bits)))
    out += [("shade_form=%d" % v, tuning(shade_form=v)) for v in (1, 2)]
    out += [("park_block=%d" % v, tuning(park_block=v)) for v in (256, 512, 1024)]
    out += [("park_dynamic=%d" % v, tuning(park_dynamic=v)) for v in (0, 1)]
    return out


def render_kinds():
    """[(name, render desc, adaptive desc or None, routed)] at the table's film size"""
    api = _api()

    def rd(spp=10, **kw):
        return api.render_desc(WIDTH, HEIGHT, spp, 6, **{"light_samples": 2, **kw})
    return [("plain_ls0", rd(light_samples=0), None, False), ("plain_ls2", rd(), None, False), ("hero4", rd(hero_wavelengths=4), None, False),
            ("medium_aware", rd(medium_aware=True), None, False), ("adaptive", rd(), api.AdaptiveDesc(40, 20, 0.05, 0.0), False), ("routed", rd(), None, True),
            ("spp40", rd(spp=40), None, False)]   # (spp40 runs under batch_slots 1024: see rows_of)


def scenes():
    """[(name, function that makes the description, literal)]: every named scene with literal rows, one fuzz seed of each class as a digest"""
    out = [(name, make, True) for name, make in scene_blob_cases.named_scenes().items()]
    out += [("fuzz_%d" % seed, (lambda seed=seed: fuzz_scenes.random_scene(seed)), False) for seed in FUZZ_SEEDS]
    return out


def load():
    """The emulation library, and the two plan exports bound with plain ctypes."""
    api = _api()
    emu, raw = scene_blob_cases.load()
    raw.ptemu_plan_scene.restype = None
    raw.ptemu_plan_scene.argtypes = [C.c_void_p, C.POINTER(api.Tuning), C.POINTER(C.c_uint32)]
    raw.ptemu_plan_render.restype = C.c_int32
    raw.ptemu_plan_render.argtypes = [C.c_void_p, C.POINTER(api.Tuning), C.c_int, C.POINTER(api.RenderDesc), C.POINTER(api.AdaptiveDesc), C.c_int, C.POINTER(C.c_uint32)]
    return emu, raw


def plan_scene(raw, scene, tn):
    """{flags, lacks, lds_mode}: plan_scene's answer for the scene under the tuning"""
    out = (C.c_uint32 * 3)()
    raw.ptemu_plan_scene(scene.handle, C.byref(tn), out)
    return dict(zip(("flags", "lacks", "lds_mode"), (int(v) for v in out)))


def plan_render(raw, scene, tn, rd, adaptive=None, routed=False, num_cus=NUM_CUS):
    """{field: value}: plan_render's answer, or the pt_status of its refusal"""
    out = (C.c_uint32 * len(FIELDS))()
    status = raw.ptemu_plan_render(scene.handle, C.byref(tn), num_cus, C.byref(rd), None if adaptive is None else C.byref(adaptive), int(routed), out)
    return status if status != 0 else dict(zip(FIELDS, (int(v) for v in out)))


def _text(column, value):
    return _NAMED[column][value] if column in _NAMED else ("0x%x" % value if column in _HEX else str(value))


def rows_of(raw, name, scene):
    """The table's rows of one scene: every render kind under every tuning, as tuples of strings in COLUMNS' order"""
    rows = []
    for tname, tn in tunings():
        flags = plan_scene(raw, scene, tn)["flags"]
        for kname, rd, adaptive, routed in render_kinds():
            used = tn
            if kname == "spp40":   # (40 spp of 3072 pixels in passes of 1024 slots: the passes overlap)
                used = type(tn).from_buffer_copy(tn)
                used.batch_slots = 1024
            plan = plan_render(raw, scene, used, rd, adaptive, routed)
            assert isinstance(plan, dict), "plan_render refused %s %s %s: status %r" % (name, kname, tname, plan)
            rows.append((name, kname, tname, _text("flags", flags)) + tuple(_text(f, plan[f]) for f in FIELDS))
    return rows


HEADER = ("# scene, render kinds, tunings, fields.  A scene's first line gives every field; the default line of each further kind gives the fields that differ from",
          "# that first line.  Every other line gives, for the kinds (*: every kind) and the tunings it names, the fields that differ from the kind's default line.  A tuning that",
          "# no line names for a kind chooses what the default chooses.  fuzz_*: one SHA-256 over the seed's full rows (" + ", ".join(COLUMNS) + ").")


def _differing(row, base):
    return " ".join("%s=%s" % (c, v) for c, v, b in zip(COLUMNS[3:], row[3:], base[3:]) if v != b)


def compact(rows):
    """The literal lines of one scene's rows (rows_of), as HEADER describes them"""
    scene, kinds, names = rows[0][0], list(dict.fromkeys(r[1] for r in rows)), list(dict.fromkeys(r[2] for r in rows))
    at = {(r[1], r[2]): r for r in rows}
    first = at[kinds[0], "default"]
    lines = ["\t".join((scene, k, "default", _differing(at[k, "default"], ("",) * len(COLUMNS) if k == kinds[0] else first))) for k in kinds]
    merged = {}   # (differing fields, the tunings that change them so) -> the kinds where they do
    for k in kinds:
        groups = {}
        for t in names:
            groups.setdefault(_differing(at[k, t], at[k, "default"]), []).append(t)
        for fields, tunings_ in groups.items():
            if fields:
                merged.setdefault((fields, ",".join(tunings_)), []).append(k)
    return lines + ["\t".join((scene, "*" if ks == kinds else ",".join(ks), tunings_, fields)) for (fields, tunings_), ks in merged.items()]


def expand(lines):
    """compact's inverse over the literal lines of a table: the full rows, as tuples in COLUMNS' order"""
    names, first, default, cells = [t for t, _ in tunings()], {}, {}, {}
    for scene, kinds, who, fields in (line.split("\t") for line in lines):
        changed = dict(f.split("=", 1) for f in fields.split())
        if who == "default":
            default[scene, kinds] = {**first.setdefault(scene, changed), **changed}
        else:
            of = [k for s, k in default if s == scene] if kinds == "*" else kinds.split(",")   # (a scene's default lines stand in front of its others)
            cells.update({(scene, k, t): changed for k in of for t in who.split(",")})
    return [(scene, kind, t) + tuple({**base, **cells.get((scene, kind, t), {})}[c] for c in COLUMNS[3:]) for (scene, kind), base in default.items() for t in names]


def table(emu, raw, full=None):
    """The lines of tests/golden/render_plans.tsv: HEADER, the named scenes' lines, and per fuzz seed one SHA-256 over its rows.  full: a list that takes the
    named scenes' full rows."""
    lines = list(HEADER)
    for name, make, literal in scenes():
        scene = emu.create_scene(make())
        rows = rows_of(raw, name, scene)
        scene.close()
        if literal and full is not None:
            full += rows
        lines += compact(rows) if literal else ["%s\tsha256\t%d\t%s" % (name, len(rows), hashlib.sha256("\n".join("\t".join(r) for r in rows).encode()).hexdigest())]
    return lines
