"""Light groups (include/pt_light_groups.h): per-group films from one render, mixed on the GPU.

The oracle of a group film is a render the parity suite already judges: group g's film is pt_render of the same scene with every emitter outside g emitting a
zero curve (scene.light_groups_room(emit=...)), bit for bit, because the walk never looks at an emission value.  The CPU tier checks the host emulation
(tests/host_emulation/ptemu_light_groups.cpp: the routed render's pass loop, ptemu_routed_pass.h, with the engine's GroupRouter) against ptemu_render and against the oracle of the masked
scenes, the mix rule against a numpy restatement, every refusal, the header and the command line; the GPU tier checks the engine against its own pt_render of
the masked scenes, against the emulation, under pass overlap, and the two mix entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emulation
import parity_suite as ps
from util import bits, film_metrics, ptcli, same_bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "pt_light_groups.h")
f32 = np.float32

# light_groups_room: instance 1 is the rect lamp, instance 2 the disk lamp; every emitter a group of its own, the environment the third
ROOM_GROUPS, ROOM_ENV_GROUP = (0, 0, 1, 0, 0, 0), 2
ONLY = [tuple(k == g for k in range(3)) for g in range(3)]   # emit = only emitter g


def room_rd(pkg):
    return pkg.api.render_desc(24, 24, 23, 5, light_samples=2, seed=7)


def counters(p):
    return (p.camera_rays, p.bounce_rays, p.shadow_rays, p.env_hits)


@pytest.fixture(scope="session")
def emu_lg(pkg):
    """The host emulation (ptemu.cpp) with the light-group render and mix (ptemu_light_groups.cpp) beside it: a library of its own."""
    return emulation.load(pkg, "light_groups")


@pytest.fixture(scope="session")
def room_emu(pkg, emu_lg):
    """The emulation's renders of the room, made once and left unchanged: the group render (total, groups, profile), ptemu_render of the complete scene and of
    the three single-emitter scenes."""
    rd = room_rd(pkg)
    film, groups, prof = emu_lg.create_scene(pkg.scene.light_groups_room()).render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    complete = emu_lg.create_scene(pkg.scene.light_groups_room()).render(rd)
    masked = [emu_lg.create_scene(pkg.scene.light_groups_room(emit=e)).render(rd) for e in ONLY]
    for a in (film, groups, complete[0]) + tuple(m[0] for m in masked):
        a.setflags(write=False)
    return {"film": film, "groups": groups, "prof": prof, "complete": complete, "masked": masked}


def mix_numpy(films, m):
    """The mix rule restated: per channel the f32 fold over g ascending of acc + ((m[g,c,0] * X_g + m[g,c,1] * Y_g) + m[g,c,2] * Z_g); w = 0."""
    films, m = np.asarray(films, f32), np.asarray(m, f32)
    G, H, W, _ = films.shape
    out = np.zeros((H, W, 4), f32)
    for c in range(3):
        acc = np.zeros((H, W), f32)
        for g in range(G):
            acc = acc + ((m[g, c, 0] * films[g, ..., 0] + m[g, c, 1] * films[g, ..., 1]) + m[g, c, 2] * films[g, ..., 2])
        out[..., c] = acc
    return out


def mix_case(w, h, G, seed):
    """Random finite films (w = 0, as a film has it) and matrices with negative and zero entries."""
    rng = np.random.default_rng(seed)
    films = (rng.random((G, h, w, 4), dtype=f32) * f32(3.0) - f32(0.5)).astype(f32)
    films[..., 3] = 0.0
    films[0, 0, 0, :3] = 0.0
    m = (rng.random((G, 3, 3), dtype=f32) * f32(4.0) - f32(2.0)).astype(f32)
    m[rng.random((G, 3, 3)) < 0.25] = 0.0
    m[G - 1, 1, 1] = -1.5
    m[0, 0, 2] = 0.0
    return films, m


MIX_SHAPES = [(17, 13), (64, 4)]
MIX_GROUPS = [1, 3, 8]


# ------------------------------------------------------------------------------------------------ CPU tier
def test_emulation_total_and_groups_are_the_masked_renders(room_emu):
    """The total film is ptemu_render's bit for bit, every group film ptemu_render's of the scene with only that emitter, and no render's walk differs."""
    e = room_emu
    assert same_bits(e["film"], e["complete"][0])
    assert counters(e["prof"]) == counters(e["complete"][1])
    for g in range(3):
        assert same_bits(e["groups"][g], e["masked"][g][0]), g
        assert counters(e["masked"][g][1]) == counters(e["prof"]), g
        assert float(e["groups"][g][..., :3].max()) > 0.0, g
    assert np.isfinite(e["groups"]).all() and not e["groups"][..., 3].any()


def test_emulation_all_dark_is_zero(pkg, emu_lg, room_emu):
    film, prof = emu_lg.create_scene(pkg.scene.light_groups_room(emit=(False, False, False))).render(room_rd(pkg))
    assert not film.any() and counters(prof) == counters(room_emu["prof"])


def test_group_films_against_the_oracle(pkg, oracle, room_emu):
    """Each group film within the project's film bar (parity_suite: L-inf < 1e-4, relative < 2e-5) of the ORACLE's film of the same masked scene."""
    rd = room_rd(pkg)
    for g in range(3):
        ref, rprof = oracle.create_scene(pkg.scene.light_groups_room(emit=ONLY[g])).render(rd)
        m = film_metrics(room_emu["groups"][g], ref)
        print("group %d vs oracle: L-inf %.3e relative %.3e" % (g, m["linf"], m["relative"]))
        assert np.isfinite(ref).all()
        assert m["linf"] < ps.FILM_LINF and m["relative"] < ps.FILM_REL, (g, m)
        assert counters(rprof) == counters(room_emu["prof"]), g


def test_one_group_is_the_total(pkg, emu_lg, room_emu):
    film, groups, _ = emu_lg.create_scene(pkg.scene.light_groups_room()).render_light_groups(room_rd(pkg), (0,) * 6, 0, groups=1)
    assert groups.shape[0] == 1 and same_bits(groups[0], film) and same_bits(film, room_emu["film"])


def test_empty_group_is_zero(pkg, emu_lg, room_emu):
    film, groups, _ = emu_lg.create_scene(pkg.scene.light_groups_room()).render_light_groups(room_rd(pkg), (0,) * 6, 0, groups=2)
    assert not groups[1].any() and same_bits(groups[0], film) and same_bits(film, room_emu["film"])


def test_groups_sum_to_the_total(room_emu):
    """The sum of the group films in f64 within the film bar of the total (measured on the host emulation: L-inf 8.4e-8, relative 2.7e-7)."""
    total = room_emu["groups"].astype(np.float64).sum(axis=0)
    m = film_metrics(total, room_emu["film"])
    print("sum of groups vs total: L-inf %.3e relative %.3e" % (m["linf"], m["relative"]))
    assert m["linf"] < ps.FILM_LINF and m["relative"] < ps.FILM_REL, m


def test_emulation_passes_keep_the_bits(pkg, emu_lg, room_emu, monkeypatch):
    """PTEMU_BATCH forces several passes (pixel chunks and sample ranges): the same films, bit for bit."""
    monkeypatch.setenv("PTEMU_BATCH", "2048")
    film, groups, prof = emu_lg.create_scene(pkg.scene.light_groups_room()).render_light_groups(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP)
    assert same_bits(film, room_emu["film"]) and same_bits(groups, room_emu["groups"]) and counters(prof) == counters(room_emu["prof"])


@pytest.mark.parametrize("G", MIX_GROUPS)
@pytest.mark.parametrize("shape", MIX_SHAPES)
def test_emulation_mix_is_the_rule(emu_lg, shape, G):
    films, m = mix_case(shape[0], shape[1], G, 100 * G + shape[0])
    assert same_bits(emu_lg.light_groups_mix(films, m), mix_numpy(films, m))


def test_mix_identity_returns_the_film(pkg, emu_lg):
    films, _ = mix_case(17, 13, 1, 5)
    films[..., 3] = 7.0   # (whatever w holds, the mix writes 0)
    out = emu_lg.light_groups_mix(films, pkg.api.light_group_gains([1.0]))
    assert same_bits(out[..., :3], films[0, ..., :3]) and not out[..., 3].any()
    assert same_bits(pkg.api.light_group_gains([2.0, 0.0]), np.stack([2 * np.eye(3, dtype=f32), np.zeros((3, 3), f32)]))


def test_refusals(pkg, emu_lg):
    """Every refusal returns its status and a message of its own."""
    a = pkg.api
    sc = emu_lg.create_scene(pkg.scene.light_groups_room())
    ok = dict(width=8, height=8, spp=10, max_bounces=3)
    cases = [
        ("group_count 0", a.render_desc(**ok), (0,) * 6, 0, 0, 1, "group_count"),
        ("group_count 9", a.render_desc(**ok), (0,) * 6, 0, 9, 1, "group_count"),
        ("group id", a.render_desc(**ok), (0, 0, 2, 0, 0, 0), 0, 2, 1, "instance 2"),
        ("environment id", a.render_desc(**ok), (0,) * 6, 3, 3, 1, "environment_group"),
        ("instance_count", a.render_desc(**ok), (0,) * 5, 0, 1, 1, "instance_count"),
        ("hero", a.render_desc(hero_wavelengths=4, **ok), (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "one wavelength"),
        ("medium", a.render_desc(medium_aware=True, **ok), (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "medium-aware"),
        ("shard", a.render_desc(shard=(0, 2), **ok), (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "whole film"),
        ("range", a.render_desc(first_sample=0, sample_count=5, **ok), (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "whole sample range"),
    ]
    seen = set()
    for name, rd, ids, env, G, status, word in cases:
        with pytest.raises(a.PtError) as e:
            sc.render_light_groups(rd, ids, env, groups=G)
        assert e.value.status == status and word in str(e.value), (name, str(e.value))
        seen.add(str(e.value))
    assert len(seen) == 8   # (the two group_count cases share a message)
    films, m = mix_case(4, 4, 2, 1)
    bad = m.copy(); bad[1, 2, 0] = np.inf
    with pytest.raises(a.PtError) as e:
        emu_lg.light_groups_mix(films, bad)
    assert e.value.status == 1 and "not finite" in str(e.value)
    # the product runs the same checks before it looks for a device: without a scene the first of them is the one that can be seen
    L = pkg.load()
    rd, gd = a.render_desc(**ok), a.LightGroupsDesc(1, 0, None, 0)
    film = np.zeros((8, 8, 4), f32)
    assert L._render_light_groups(None, C.byref(rd), C.byref(gd), film.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 1
    assert L.last_error() == "the scene is null"
    assert L._light_groups_mix(4, 4, 9, films.ctypes.data_as(C.POINTER(C.c_float)), m.ctypes.data_as(C.POINTER(C.c_float)), film.ctypes.data_as(C.POINTER(C.c_float))) == 1
    assert "group_count" in L.last_error()


def test_header_is_exported_and_the_desc_has_the_compilers_size(pkg, tmp_path):
    text = open(HEADER).read()
    names = re.findall(r"^pt_status (pt_\w+)\(", text, re.M)
    assert sorted(names) == ["pt_light_groups_mix", "pt_light_groups_mix_resident", "pt_light_groups_resident", "pt_render_light_groups"]
    lib = C.CDLL(pkg.load().path)
    for n in names:
        assert getattr(lib, n) is not None
    assert "#define PT_LIGHT_GROUPS_MAX 8" in text and pkg.api.LIGHT_GROUPS_MAX == 8
    src = tmp_path / "size.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_light_groups.h"\nint main(void) { printf("%zu %zu %zu", sizeof(pt_light_groups_desc), '
                   'offsetof(pt_light_groups_desc, instance_group), offsetof(pt_light_groups_desc, environment_group)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off_ids, off_env = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    D = pkg.api.LightGroupsDesc
    assert (C.sizeof(D), D.instance_group.offset, D.environment_group.offset) == (size, off_ids, off_env)


def scaled_c2_config(pkg):
    """data/config_cornell_c2.toml at 32x32 and 20 spp, with a premultiply so that the factor of the EXR payload is not 1."""
    text = open(os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c2.toml")).read()
    text, n1 = re.subn(r"min_samples = \d+", "min_samples = 20", text)
    text, n2 = re.subn(r"width = \d+\nheight = \d+", "width = 32\nheight = 32", text)
    text, n3 = re.subn(r"only_direct = false\n", "only_direct = false\npremultiply = 2.0\n", text)
    assert (n1, n2, n3) == (1, 1, 1)
    return text


def test_ptcli_flags_while_parsing(pkg):
    """Each forbidden combination exits with status 2 and its own message before any file is read; the help and the file's head name the flags."""
    exe = ptcli(pkg)
    lg = ["--light-groups", "instance"]
    cases = [(lg + extra, "--light-groups cannot be combined with " + extra[0]) for extra in (
        ["--adaptive", "0.1"], ["--denoise"], ["--spectral-bins", "8"], ["--denoise-spectral-bins", "8"], ["--devices", "1"], ["--spectral-devices", "1"],
        ["--hero-wavelengths", "4"])]
    cases += [
        (["--light-groups", "face"], "--light-groups needs `instance` or `material`"),
        (["--light-groups"], "--light-groups needs a value"),
        (["--light-gains", "1,2"], "--light-gains needs --light-groups"),
        (lg + ["--light-gains", "1,x"], "--light-gains needs finite gains"),
        (lg + ["--light-gains", "1,,2"], "--light-gains needs finite gains"),
        (lg + ["--light-gains", "1,2,3,4,5,6,7,8,9"], "--light-gains takes at most 8 gains"),
    ]
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
    assert "[--light-groups instance|material] [--light-gains G0,G1,...]" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    head = open(os.path.join(CSRC, "host", "ptcli.cpp")).read().split("#include")[0]
    assert "[--light-groups instance|material] [--light-gains G0,G1,...]" in head


def test_ptcli_dry_run_accepts_the_flags(pkg, tmp_path):
    """A dry run loads the scene, forms the groups and ends well; gains that do not match the groups end it with a message."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n"]
    for mode in ("instance", "material"):
        ok = subprocess.run(base + ["--light-groups", mode], capture_output=True, text=True, cwd=str(tmp_path))
        assert ok.returncode == 0 and re.search(r"light groups: \d+ ", ok.stdout), (ok.stdout, ok.stderr)
    G = int(re.search(r"light groups: (\d+) ", ok.stdout).group(1))
    ok = subprocess.run(base + ["--light-groups", "instance", "--light-gains", ",".join(["1.5"] * G)], capture_output=True, text=True, cwd=str(tmp_path))
    assert ok.returncode == 0, ok.stderr
    bad = subprocess.run(base + ["--light-groups", "instance", "--light-gains", ",".join(["1.5"] * (G + 1))], capture_output=True, text=True, cwd=str(tmp_path))
    assert bad.returncode == 1 and "--light-gains needs one gain per group" in bad.stderr, bad.stderr


# ------------------------------------------------------------------------------------------------ GPU tier
def clean_tuning(engine, pkg, batch_slots=0, flags=0):
    t = engine.tuning_default()
    t.flags &= ~(pkg.api.TUNE_NO_PASS_OVERLAP | pkg.api.TUNE_NO_LDS | pkg.api.TUNE_PASS_SKEW_MASK << pkg.api.TUNE_PASS_SKEW_SHIFT)   # (whatever the environment holds)
    t.flags |= flags
    t.batch_slots = batch_slots
    return t


@pytest.fixture(scope="module")
def room_gpu(engine, pkg):
    """The engine's renders of the room on one scene handle, made once: pt_render before, the group render, pt_render after; and pt_render of the masked scenes."""
    rd = room_rd(pkg)
    sc = engine.create_scene(pkg.scene.light_groups_room())
    before = sc.render(rd)
    film, groups, prof = sc.render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    after = sc.render(rd)
    masked = [engine.create_scene(pkg.scene.light_groups_room(emit=e)).render(rd) for e in ONLY]
    return {"scene": sc, "before": before, "after": after, "film": film, "groups": groups, "prof": prof, "masked": masked}


@pytest.mark.gpu
def test_gpu_film_is_pt_renders(room_gpu):
    g = room_gpu
    assert same_bits(g["film"], g["before"][0]) and counters(g["prof"]) == counters(g["before"][1])


@pytest.mark.gpu
def test_gpu_groups_are_the_masked_renders_and_the_emulations(room_gpu, room_emu):
    g = room_gpu
    assert np.isfinite(g["groups"]).all()
    for k in range(3):
        assert same_bits(g["groups"][k], g["masked"][k][0]), k
        assert counters(g["masked"][k][1]) == counters(g["prof"]), k
    assert same_bits(g["groups"], room_emu["groups"]) and same_bits(g["film"], room_emu["film"])
    assert counters(g["prof"]) == counters(room_emu["prof"])


@pytest.mark.gpu
def test_gpu_pt_render_before_and_after(room_gpu):
    """pt_render on the same scene handle before and after a group render: the same bits (the wider energy buffer and the group films disturb nothing)."""
    g = room_gpu
    assert same_bits(g["before"][0], g["after"][0]) and counters(g["before"][1]) == counters(g["after"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["overlap", "no_overlap", "no_lds"])
def test_gpu_passes_and_tunings_keep_the_bits(engine, pkg, room_gpu, variant):
    """pt_tuning::batch_slots 2048 cuts the render into passes of at most 204 pixels x 10 samples (three pixel chunks x three sample ranges), so both sets of pass
    buffers are used, each more than once, every pixel is continued by later passes and k_accumulate_groups' cross-pass order matters; likewise without the
    overlap and without LDS staging."""
    flags = {"overlap": 0, "no_overlap": pkg.api.TUNE_NO_PASS_OVERLAP, "no_lds": pkg.api.TUNE_NO_LDS}[variant]
    sc = engine.create_scene(pkg.scene.light_groups_room(), tuning=clean_tuning(engine, pkg, 2048, flags))
    film, groups, prof = sc.render_light_groups(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP)
    print("passes:", prof.kernel_launches[0])
    assert prof.kernel_launches[0] >= 7
    assert same_bits(film, room_gpu["film"]) and same_bits(groups, room_gpu["groups"]) and counters(prof) == counters(room_gpu["prof"])


def emissive_mesh_scene(pkg, mesh=True, rect=True):
    """scene.hdri_emissive_mesh with a second light instance, a rect lamp of a material of its own.  Its HDRI cannot be masked by a zero curve — the importance
    map is baked from the environment's own emission, so a dark environment is another walk — and so the two groups compared against masked renders are the
    two instances: the mesh whose instance carries a light material, and the rect.  mesh / rect False: that emitter's emission curve is flat_zero."""
    sm = pkg.scene
    b = sm.hdri_test(mesh=None, hdri_size=(64, 32), importance=(32, 32))
    sm.add_library_curves(b, ["flat_zero", "E5", "E10", "flat_78"])
    zero = b.curve("flat_zero")
    lamp = b.material_diffuse_light("lg_mesh_lamp", b.curve("E5") if mesh else zero, b.curve("flat_78"), pkg.api.SIDED_DUAL)
    p, f, n, _ = sm._npz_mesh("gem")
    m = b.add_mesh(p, f, n, face_materials=pkg.api.material_id(pkg.api.TAG_MATERIAL, 0))
    b.add_mesh_instance(m, lamp, sm.transform_from_data(scale=(0.5, 0.5, 0.5), translate=(-0.6, 1.5, -0.1)))
    lamp2 = b.material_diffuse_light("lg_rect_lamp", b.curve("E10") if rect else zero, b.curve("flat_78"), pkg.api.SIDED_DUAL)
    b.add_rect((0.6, 0.6), (0.4, -1.0, 1.2), "Z", True, lamp2)
    return b


EM_RD = dict(width=16, height=16, spp=12, max_bounces=5, light_samples=2, seed=3)


def emissive_mesh_identities(lib, pkg):
    """What holds bit for bit on `lib` (the emulation or the engine) for emissive_mesh_scene, whose last two instances are the mesh and the rect:
    the three-way grouping (environment 0, mesh 1, rect 2); the environment's film is the plain render with both instances dark; with the mesh alone in
    group 1 the rest — group 0 — is the plain render with the mesh dark and group 1 the mesh's film, and likewise for the rect; no walk differs.
    Returns the three-way render."""
    rd = pkg.api.render_desc(**EM_RD)
    b = emissive_mesh_scene(pkg)
    n = len(b.instances)
    three = [0] * n; three[n - 2], three[n - 1] = 1, 2
    sc = lib.create_scene(b)
    film, groups, prof = sc.render_light_groups(rd, three, 0)
    plain, pprof = sc.render(rd)
    assert same_bits(film, plain) and counters(prof) == counters(pprof)
    assert np.isfinite(groups).all() and all(float(groups[g][..., :3].max()) > 0.0 for g in range(3))
    dark, dprof = lib.create_scene(emissive_mesh_scene(pkg, mesh=False, rect=False)).render(rd)
    assert same_bits(groups[0], dark) and counters(dprof) == counters(prof)
    for at, g, kw in ((n - 2, 1, dict(mesh=False)), (n - 1, 2, dict(rect=False))):
        ids = [0] * n; ids[at] = 1
        _, two, _ = sc.render_light_groups(rd, ids, 0)
        masked, mprof = lib.create_scene(emissive_mesh_scene(pkg, **kw)).render(rd)
        assert same_bits(two[0], masked) and counters(mprof) == counters(prof), g
        assert same_bits(two[1], groups[g]), g
    return film, groups, prof


def test_emissive_mesh_scene_masks_on_the_emulation(pkg, emu_lg):
    """The masked scenes of the GPU test, verified on the emulation first."""
    emissive_mesh_identities(emu_lg, pkg)


@pytest.mark.gpu
def test_gpu_emissive_mesh_and_a_second_light(engine, pkg, emu_lg):
    """hdri_emissive_mesh at 16 x 16, 12 spp with a second light instance (its HDRI cannot be masked by a zero curve, emissive_mesh_scene): the identities of
    emissive_mesh_identities on the engine — the general forms with emissive mesh hits, certificates and an importance-sampled environment — and the emulation's bits."""
    film, groups, prof = emissive_mesh_identities(engine, pkg)
    b = emissive_mesh_scene(pkg)
    n = len(b.instances)
    three = [0] * n; three[n - 2], three[n - 1] = 1, 2
    efilm, egroups, eprof = emu_lg.create_scene(b).render_light_groups(pkg.api.render_desc(**EM_RD), three, 0)
    assert same_bits(film, efilm) and same_bits(groups, egroups) and counters(prof) == counters(eprof)


@pytest.mark.gpu
@pytest.mark.parametrize("G", MIX_GROUPS)
@pytest.mark.parametrize("shape", [(17, 13), (24, 24)])
def test_gpu_mix_is_the_rule(engine, shape, G):
    films, m = mix_case(shape[0], shape[1], G, 100 * G + shape[0])
    assert same_bits(engine.light_groups_mix(films, m), mix_numpy(films, m))


@pytest.mark.gpu
@pytest.mark.parametrize("G", MIX_GROUPS)
@pytest.mark.parametrize("shape", [(17, 13), (24, 24)])
def test_gpu_mix_resident_is_the_rule(engine, pkg, shape, G):
    """pt_light_groups_mix_resident over the films a group render of that size and G left on the device: the numpy rule over the films it returned, bit for bit
    (the room's six instances dealt over the G groups, the environment in the last)."""
    sc = engine.create_scene(pkg.scene.light_groups_room())
    _, groups, _ = sc.render_light_groups(pkg.api.render_desc(shape[0], shape[1], 10, 4, light_samples=2, seed=G), [i % G for i in range(6)], G - 1, groups=G)
    assert sc.light_groups_resident() == (shape[0], shape[1], G) and float(groups[G - 1][..., :3].max()) > 0.0
    _, m = mix_case(shape[0], shape[1], G, 7 * G + shape[1])
    assert same_bits(sc.light_groups_mix_resident(m), mix_numpy(groups, m))


@pytest.mark.gpu
def test_gpu_mix_resident(engine, pkg, room_gpu):
    """The resident mix equals the numpy rule over the films the render returned; after a second group render (another size, another G) it uses that
    render's films; read_groups False leaves the films on the device alone."""
    sc = room_gpu["scene"]
    assert sc.light_groups_resident() == (24, 24, 3)
    _, m = mix_case(24, 24, 3, 11)
    assert same_bits(sc.light_groups_mix_resident(m), mix_numpy(room_gpu["groups"], m))
    gains = pkg.api.light_group_gains([0.0, 2.0, 0.5])
    assert same_bits(sc.light_groups_mix_resident(gains), mix_numpy(room_gpu["groups"], gains))
    fresh = engine.create_scene(pkg.scene.light_groups_room())
    assert fresh.light_groups_resident() is None
    with pytest.raises(pkg.api.PtError) as e:
        fresh.light_groups_mix_resident(gains)
    assert "no resident group films" in str(e.value)
    rd2 = pkg.api.render_desc(17, 13, 10, 4, light_samples=1, seed=2)
    ids8 = (0, 1, 2, 3, 4, 5)
    film8, groups8, _ = fresh.render_light_groups(rd2, ids8, 7, groups=8)
    assert fresh.light_groups_resident() == (17, 13, 8)
    _, m8 = mix_case(17, 13, 8, 12)
    assert same_bits(fresh.light_groups_mix_resident(m8), mix_numpy(groups8, m8))
    _, none, _ = fresh.render_light_groups(room_rd(pkg), (0,) * 6, 0, groups=1, read_groups=False)
    assert none is None and fresh.light_groups_resident() == (24, 24, 1)
    assert same_bits(fresh.light_groups_mix_resident(pkg.api.light_group_gains([1.0]))[..., :3], room_gpu["film"][..., :3])


@pytest.mark.gpu
def test_gpu_ptcli_light_groups(pkg, tmp_path):
    """ptcli --light-groups instance --light-gains: the usual files byte for byte those of a run without the flags, one EXR per group, and the relit pair."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    dry = run("dry", "-n", "--light-groups", "instance")
    G = int(re.search(r"light groups: (\d+) ", dry.stdout).group(1))
    plain, lit = run("plain"), run("lit", "--light-groups", "instance", "--light-gains", ",".join(["0.5"] * G))
    assert plain.returncode == 0 and lit.returncode == 0, (plain.stderr, lit.stderr)
    usual = sorted(os.listdir(tmp_path / "plain"))
    assert usual and all(open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "lit" / f, "rb").read() for f in usual)
    extra = sorted(set(os.listdir(tmp_path / "lit")) - set(usual))
    stem = usual[0].rsplit(".", 1)[0]
    assert extra == sorted(["%s_light%d.exr" % (stem, g) for g in range(G)] + [stem + "_relit.exr", stem + "_relit.png"]), extra
