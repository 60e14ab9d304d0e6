"""Emissive triangle meshes as lights ("an emissive mesh face"): every emissive face is a light-list entry of its own, sampled
with the square-root mapping over the face, area pdf 1 / A_f.  The reference cannot render these scenes (its MeshTriangleRef::sample is todo!()),
so there is no oracle: the CPU tier checks the sampler bit for bit against a float32 restatement of the definition and the film under the
emulation's switches; the GPU tier compares estimators whose expectations agree, forms that must agree bit for bit, and the GPU with the emulation."""
import os

import numpy as np
import pytest

import emulation

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32

# the Cornell box's lamp (scene.cornell_box): a one-sided rect, normal +z
LAMP_SIZE, LAMP_ORIGIN = (0.105, 0.13), (0.278, 0.2795, 0.5487)


@pytest.fixture(scope="session")
def emu_ml(pkg):
    """The host emulation (tests/host_emulation/ptemu.cpp) with the light sampler's export (ptemu_light.cpp) beside it: a library of its own."""
    return emulation.load(pkg, "mesh_lights")


# ------------------------------------------------------------------------------------------------ scenes
def quad(size, centre, z_up=True):
    """Two triangles over the rect of `size` centred at `centre` in the plane z = centre.z, face normal +z (or -z)."""
    (w, h), (cx, cy, cz) = size, centre
    p = np.array([[cx - w / 2, cy - h / 2, cz], [cx + w / 2, cy - h / 2, cz], [cx + w / 2, cy + h / 2, cz], [cx - w / 2, cy + h / 2, cz]], f32)
    f = np.array([[0, 1, 2], [0, 2, 3]] if z_up else [[0, 2, 1], [0, 3, 2]], np.uint32)
    return p, f


def dome(rings=3, segs=8, radius=0.06):
    """A smooth-shaded cap (a tessellated lamp opening downward) with vertex normals pointing up and in — the Cornell light emits on the reverse side, down and out."""
    p, n = [(0.0, 0.0, 0.0)], [(0.0, 0.0, 1.0)]
    for r in range(1, rings + 1):
        th = 0.5 * np.pi * r / rings * 0.8
        for s in range(segs):
            ph = 2 * np.pi * s / segs
            d = (np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th))
            p.append((radius * d[0], radius * d[1], radius * (1.0 + d[2]) * 0.5))
            n.append((-d[0], -d[1], -d[2]))
    f = []
    for s in range(segs):
        f.append((0, 1 + (s + 1) % segs, 1 + s))
    for r in range(1, rings):
        a, b = 1 + (r - 1) * segs, 1 + r * segs
        for s in range(segs):
            s1 = (s + 1) % segs
            f += [(a + s, a + s1, b + s1), (a + s, b + s1, b + s)]
    return np.asarray(p, f32), np.asarray(f, np.uint32), np.asarray(n, f32)


def lamp_transform(pkg):
    """A rotation and a translation that hang a lamp built at the origin below the Cornell box's ceiling, tilted."""
    return pkg.scene._mat4_mul(pkg.scene.transform_from_translation((0.278, 0.2795, 0.5)), pkg.scene.transform_from_axis_angle((0.3, 1.0, 0.2), 0.6))


def cornell(pkg, lamp="rect", glass_body=False, light_rect_too=False):
    """The Cornell box of scene.cornell_box with its lamp replaced: "rect" (the original), "quad" (two triangles over the same rect, the same
    material), "quad_xf" (the quad built at the origin and rotated + translated into place), "dome" (a smooth-shaded tessellated lamp with vertex
    normals), "few" (a lambertian box of which two faces emit), "tri" (a single emissive triangle: the scene's only light), "rect_xf" (a rect
    lamp under quad_xf's transform)."""
    b = pkg.scene.cornell_box()
    light = b.material("diffuse_light_cornell")
    white = b.material("lambertian_white")
    b.instances.pop(0)                       # the rect lamp (instance 0 of cornell_box)
    if lamp == "rect" or light_rect_too:
        b.add_rect(LAMP_SIZE, LAMP_ORIGIN, "Z", False, light)
    if lamp == "quad":
        p, f = quad(LAMP_SIZE, LAMP_ORIGIN)
        b.add_mesh_instance(b.add_mesh(p, f, None, face_materials=light))
    elif lamp == "quad_xf":
        p, f = quad(LAMP_SIZE, (0.0, 0.0, 0.0))
        b.add_mesh_instance(b.add_mesh(p, f, None, face_materials=light), None, lamp_transform(pkg))
    elif lamp == "rect_xf":
        b.add_rect(LAMP_SIZE, (0.0, 0.0, 0.0), "Z", False, light, lamp_transform(pkg))
    elif lamp == "dome":
        p, f, n = dome()
        xf = pkg.scene.transform_from_translation((0.278, 0.2795, 0.5))
        b.add_mesh_instance(b.add_mesh(p, f, n, face_materials=light), None, xf)
    elif lamp == "few":
        p = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], f32) * f32(0.12) + np.array([0.2, 0.2, 0.2], f32)
        f = np.array([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (1, 2, 6), (1, 6, 5), (2, 3, 7), (2, 7, 6), (3, 0, 4), (3, 4, 7)], np.uint32)
        glow = pkg.scene.add_library_material(b, "diffuse_light_flat_x5")   # (two-sided: the box's outward faces light the room)
        fm = np.full(12, white, np.uint32)
        fm[2:4] = glow                        # the top face
        fm[8] = glow                          # and one triangle of a side
        b.add_mesh_instance(b.add_mesh(p, f, None, face_materials=fm))
        b.add_rect(LAMP_SIZE, LAMP_ORIGIN, "Z", False, light)
    elif lamp == "tri":
        p = np.array([[0.2, 0.2, 0.5487], [0.36, 0.2, 0.5487], [0.28, 0.36, 0.5487]], f32)
        b.add_mesh_instance(b.add_mesh(p, np.array([[0, 1, 2]], np.uint32), None, face_materials=light))
    if glass_body:
        glass = pkg.scene.add_library_material(b, "ggx_glass_rough")
        cube = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], f32) * f32(0.15) + np.array([0.05, 0.38, 0.05], f32)
        cf = np.array([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (1, 2, 6), (1, 6, 5), (2, 3, 7), (2, 7, 6), (3, 0, 4), (3, 4, 7)], np.uint32)
        b.add_mesh_instance(b.add_mesh(cube, cf, None, face_materials=pkg.api.material_id(pkg.api.TAG_MATERIAL, 0)), glass)
    return b


# ------------------------------------------------------------------------------------------------ the definition, restated in float32
def _norm(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _normalize(v):
    return v / _norm(v)[..., None]


def _xf_point(m, p):
    return np.stack([m[4 * r] * p[..., 0] + m[4 * r + 1] * p[..., 1] + m[4 * r + 2] * p[..., 2] + m[4 * r + 3] for r in range(3)], -1)


def _xf_vec(m, v):
    return np.stack([m[4 * r] * v[..., 0] + m[4 * r + 1] * v[..., 1] + m[4 * r + 2] * v[..., 2] for r in range(3)], -1)


def heron(p0, p1, p2):
    """MeshTriangleRef::surface_area (mesh.rs:200-210) in float32, its order: lengths |p2 - p0|, |p1 - p0|, |p2 - p1|, s = 0.5 (d02 + d01 + d12)."""
    d02, d01, d12 = _norm(p2 - p0), _norm(p1 - p0), _norm(p2 - p1)
    s = f32(0.5) * (d02 + d01 + d12)
    return np.sqrt(s * (s - d01) * (s - d12) * (s - d02))


def sample_face(p, n, fwd, rev, frm, s2):
    """sample(s, from) of one emissive face (vertices p (3, 3), vertex normals n (3, 3) or None) of an instance (fwd / rev: its 4x4 rows, None = no
    transform), as DESIGN.md section 10 defines it, in float32: the direction (n, 3) and the solid-angle pdf (n,)."""
    p0, p1, p2 = (p[k].astype(f32) for k in range(3))
    frm = frm.astype(f32)
    if rev is not None:
        frm = _xf_point(rev, frm)
    su = np.sqrt(s2[:, 0].astype(f32))
    b0 = f32(1) - su
    b1 = s2[:, 1].astype(f32) * su
    b2 = f32(1) - b0 - b1
    point = p0 * b0[:, None] + p1 * b1[:, None] + p2 * b2[:, None]
    if n is None:
        normal = np.broadcast_to(_normalize(_normalize(np.cross(p0 - p2, p1 - p2).astype(f32))), point.shape)   # (cross: x y - y x per component, exact order)
    else:
        normal = _normalize(n[0].astype(f32) * b0[:, None] + n[1].astype(f32) * b1[:, None] + n[2].astype(f32) * b2[:, None])
    area_pdf = f32(1) / heron(p0, p1, p2)
    direction = point - frm
    dn = _normalize(direction)
    cos_i = normal[:, 0] * dn[:, 0] + normal[:, 1] * dn[:, 1] + normal[:, 2] * dn[:, 2]
    with np.errstate(all="ignore"):
        pdf = area_pdf * (direction[:, 0] * direction[:, 0] + direction[:, 1] * direction[:, 1] + direction[:, 2] * direction[:, 2]) / np.abs(cos_i)
    pdf = np.where(np.isfinite(pdf), pdf, f32(0)).astype(f32)
    if fwd is not None:
        dn = _normalize(_xf_vec(fwd, dn))
    return dn.astype(f32), pdf


def _cross_exact(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


# ------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("lamp", ["quad", "dome"])
def test_scenes_with_emissive_faces_create(emu_ml, pkg, lamp):
    """A scene with an emissive two-triangle quad and one with a smooth-shaded emissive mesh both create (before this, scene creation refused
    them: "mesh lights cannot be sampled"), with one light-list entry per emissive face."""
    sc = emu_ml.create_scene(cornell(pkg, lamp))
    info = lambda k: int(sc.library._debug_scene_info(sc.handle, k))
    faces = 2 if lamp == "quad" else len(dome()[1])
    assert info(1000000 + 9) == faces                       # PT_HDR_LIGHT_COUNT
    assert info(1000000 + 71) != 0                          # PT_HDR_LIGHT_FACE_OFF


def test_scenes_without_emissive_faces_keep_their_blob(emu_ml, pkg):
    """A scene without emissive faces has no face list (header word 71 = 0) and its light list is what it was: the Cornell box's one rect."""
    sc = emu_ml.create_scene(pkg.scene.cornell_box())
    info = lambda k: int(sc.library._debug_scene_info(sc.handle, k))
    assert info(1000000 + 71) == 0 and info(1000000 + 9) == 1


def _face_cases(pkg):
    rng = np.random.default_rng(7)
    rot = pkg.scene._mat4_mul(pkg.scene.transform_from_translation((0.3, -0.2, 0.9)), pkg.scene.transform_from_axis_angle((0.3, 1.0, 0.2), 0.6))
    p, f, n = dome()
    cases = []
    for name, (pp, ff, nn) in (("flat", (rng.uniform(-1, 1, (6, 3)).astype(f32), np.array([[0, 1, 2], [3, 4, 5], [0, 4, 2]], np.uint32), None)),
                               ("smooth", (p, f[:7], n))):
        for xf in (None, rot):
            cases.append((name, pp, ff, nn, xf))
    return cases


def test_light_sample_bit_exact_against_the_definition(emu_ml, pkg):
    """ptemu_light_sample (the vertex kernels' light_sample) equals a numpy float32 restatement of the definition, bit for bit: random faces, samples
    and origins; untransformed and rigidly transformed instances; flat and smooth faces.  The host's A_f is numpy's Heron in float32."""
    rng = np.random.default_rng(11)
    for name, p, f, n, xf in _face_cases(pkg):
        b = cornell(pkg, "rect")
        light = b.material("diffuse_light_cornell")
        b.add_mesh_instance(b.add_mesh(p, f, n, face_materials=light), None, xf)
        sc = emu_ml.create_scene(b)
        info = lambda k: int(sc.library._debug_scene_info(sc.handle, k))
        assert info(1000000 + 9) == 1 + len(f)
        fwd = rev = None
        if xf is not None:
            fwd = np.asarray(xf, np.float64).astype(f32).reshape(-1)[:12]
            rev = pkg.scene.transform_inverse(np.asarray(xf, np.float64)).astype(f32).reshape(-1)[:12]
        m = 4096
        frm = rng.uniform(-2, 2, (m, 3)).astype(f32)
        s2 = rng.uniform(0, 1, (m, 2)).astype(f32)
        s2[:4] = [[0, 0], [1, 1], [0, 1], [1, 0]]
        face_list = info(1000000 + 71)
        for j in range(len(f)):
            entry = 1 + j                      # (entry 0: the rect lamp; the mesh instance's run follows in face order)
            d, pdf = sc.light_sample(entry, frm, s2)
            nn = None if n is None else n[f[j]]
            d_ref, pdf_ref = sample_face(p[f[j]], nn, fwd, rev, frm, s2)
            assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)), (name, xf is not None, j)
            assert np.array_equal(pdf.view(np.uint32), pdf_ref.view(np.uint32)), (name, xf is not None, j)
            # the host's A_f, in the spare word of the face's normal record (pt_blob.h PT_HDR_LIGHT_FACE_OFF)
            triw = info(1000000 + face_list + entry)
            core = info(1000000 + 61)
            mesh_rec = info(1000000 + info(1000000 + 4) + (len(b.instances) - 1) * 40 + 3)
            normal_off, tri_off = info(1000000 + mesh_rec + 3), info(1000000 + mesh_rec + 2)
            spare = (normal_off + (triw - tri_off) + 3) if normal_off else (info(1000000 + core + triw + 7) + 3)
            area = np.array([info(1000000 + core + spare)], np.uint32).view(f32)[0]
            pp = p[f[j]].astype(f32)
            assert area.view(np.uint32) == heron(pp[0], pp[1], pp[2]).view(np.uint32), (name, j)
        with pytest.raises(Exception):
            sc.light_sample(1 + len(f), frm[:1], s2[:1])


def test_face_normal_restatement(pkg):
    """(the restatement's flat normal is the host's: normalize(normalize(cross(p0 - p2, p1 - p2))), cross component by component)"""
    p = np.random.default_rng(3).uniform(-1, 1, (3, 3)).astype(f32)
    assert np.array_equal(np.cross(p[0] - p[2], p[1] - p[2]).astype(f32), _cross_exact(p[0] - p[2], p[1] - p[2]))


SWITCHES = [{}, {"PTEMU_FLAGS": "2"}, {"PTEMU_FLAGS": "4"}, {"PTEMU_FLAGS": "16"}, {"PTEMU_FLAGS": "64"}, {"PTEMU_FLAGS": "256"}, {"PTEMU_FLAGS": "512"},
            {"PTEMU_FLAGS": "1024"}, {"PTEMU_FLAGS": "128"}, {"PTEMU_SHADE_FORM": "2"}, {"PTEMU_NO_CONVEX": "1"}, {"PTEMU_NO_MESH_SHORTCUTS": "1"}]


@pytest.mark.parametrize("lamp,glass,hero,medium", [("quad_xf", True, 1, False), ("tri", False, 1, False), ("dome", False, 4, False), ("few", True, 1, True)])
def test_mesh_light_films_under_the_emulations_switches(emu_ml, pkg, monkeypatch, lamp, glass, hero, medium):
    """A mesh-light scene renders bit-identically under the emulation's switch flags (exact slabs, no culling, no sweep, no mesh sweep, no known light,
    no one-light shortcut, no light pre-pass, the replayed phase 3, the full vertex form, no certificates, no mesh shortcuts): every search, bound and
    shortcut the emissive faces meet decides as the plain search does."""
    rd = pkg.api.render_desc(24, 16, 6, 5, seed=3, hero_wavelengths=hero, medium_aware=medium)
    films = []
    for env in SWITCHES:
        for k in ("PTEMU_FLAGS", "PTEMU_SHADE_FORM", "PTEMU_NO_CONVEX", "PTEMU_NO_MESH_SHORTCUTS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        film, prof = emu_ml.create_scene(cornell(pkg, lamp, glass_body=glass)).render(rd)
        films.append((env, film, prof.shadow_rays))
    base = films[0][1]
    assert np.isfinite(base).all() and base[..., 1].sum() > 0
    for env, film, _ in films[1:]:
        assert np.array_equal(base.view(np.uint32), film.view(np.uint32)), env


def test_emissive_faces_are_lights_for_the_certificates(emu_ml, pkg):
    """An instance with emissive faces counts as a light where the convex certificate asks "is a light near the body" (lightish) and gets no inner ball; a
    closed glass cube next to it still gets its certificate."""
    b = cornell(pkg, "few", glass_body=True)
    sc = emu_ml.create_scene(b)
    w = lambda k: int(sc.library._debug_scene_info(sc.handle, 1000000 + k))
    insts = w(4)
    flags = [w(insts + i * 40 + 1) for i in range(w(5))]
    meshes = [i for i in range(w(5)) if w(insts + i * 40) == pkg.api.SHAPE_MESH]
    lamp_box, glass = meshes[-2], meshes[-1]
    assert flags[lamp_box] & (16 | 32) == 0                        # the emissive box: never certified
    assert w(w(insts + lamp_box * 40 + 3) + 11) == 0               # and no inner ball (PT_MESH_INNER_R)
    assert flags[glass] & (16 | 32) != 0                           # the glass cube beside it: certified


# ------------------------------------------------------------------------------------------------ GPU tier
def _block_means(film, block=16):
    h, w = film.shape[:2]
    return film[..., :3].reshape(h // block, block, w // block, block, 3).mean(axis=(1, 3))


def _seed_stats(engine, pkg, builder, rd_of, seeds):
    sc = engine.create_scene(builder)
    blocks = np.stack([_block_means(sc.render(rd_of(s))[0].astype(np.float64)) for s in seeds])
    return blocks.mean(axis=0), blocks.std(axis=0, ddof=1) / np.sqrt(len(seeds))


def _agree(a, b, what):
    (ma, sa), (mb, sb) = a, b
    sigma = np.sqrt(sa * sa + sb * sb)
    z = np.abs(ma - mb) / np.maximum(sigma, 1e-12)
    assert ma.max() > 0 and mb.max() > 0, what
    assert (np.abs(ma - mb) <= 5.0 * sigma + 1e-7 * np.abs(ma)).all(), (what, float(z.max()))


SEEDS = list(range(1, 9))


def _direct(pkg, L, spp=512):
    """only_direct with L light samples (NEE, weight 1), no roulette."""
    return lambda s: pkg.api.render_desc(64, 64, spp, 2, min_bounces=2, light_samples=L, only_direct=True, seed=s)


@pytest.mark.gpu
def test_gpu_nee_of_the_quad_lamp_matches_the_rect_lamp(engine, pkg):
    """only_direct, L = 2: the Cornell box lit by its rect lamp and by a two-triangle mesh over the same rect with the same material — the same direct
    light in expectation (area sampling of the same surface), block by block within 5 sigma of the seed-to-seed spread (64^2 x 4096 spp each)."""
    rect = _seed_stats(engine, pkg, cornell(pkg, "rect"), _direct(pkg, 2), SEEDS)
    quad_ = _seed_stats(engine, pkg, cornell(pkg, "quad"), _direct(pkg, 2), SEEDS)
    _agree(rect, quad_, "rect vs quad")


@pytest.mark.gpu
def test_gpu_nee_of_a_transformed_quad_lamp_matches_the_transformed_rect(engine, pkg):
    """only_direct, L = 2: a rotated and translated quad lamp against a rect lamp under the same transform (the same surface, the same normal, the
    same material): the same direct light in expectation, through the Instance wrapper of both (its object-space pdf), within 5 sigma per block.
    (NEE is not compared with BSDF-sampled direct light: the kept extra light-side cosine of NEE, DESIGN.md section 10, makes the two differ — the
    rect lamp itself, the control, differs by up to a quarter per block.)"""
    rect = _seed_stats(engine, pkg, cornell(pkg, "rect_xf"), _direct(pkg, 2), SEEDS)
    quad_ = _seed_stats(engine, pkg, cornell(pkg, "quad_xf"), _direct(pkg, 2), SEEDS)
    _agree(rect, quad_, "transformed rect vs transformed quad")


TUNE_FLAGS = ["TUNE_NO_LDS", "TUNE_NO_CORE_LDS", "TUNE_NO_PARK", "TUNE_NO_LIVE_LIST", "TUNE_EXACT_SLAB", "TUNE_NO_CULL", "TUNE_NO_SWEEP", "TUNE_NO_MESH_SWEEP",
              "TUNE_NO_KNOWN_LIGHT", "TUNE_GENERAL_FORMS", "TUNE_NO_FUSE", "TUNE_NO_STAGE_TIMING", "TUNE_NO_AXIS_SCAN", "TUNE_NO_ONE_LIGHT", "TUNE_NO_CONVEX",
              "TUNE_NO_MESH_SHORTCUTS"]


@pytest.mark.gpu
@pytest.mark.parametrize("lamp,glass,hero,medium", [("quad_xf", True, 1, False), ("tri", False, 1, False), ("dome", False, 4, False), ("few", True, 4, False),
                                                    ("few", True, 1, True)])
def test_gpu_mesh_light_films_are_bit_identical_under_every_switch(engine, pkg, lamp, glass, hero, medium):
    """A mesh-light film is the same bit for bit under every PT_TUNE_* switch (NO_ONE_LIGHT on the single-emissive-triangle scene, NO_CONVEX with a
    certified glass body next to the lamp, GENERAL_FORMS), with light_prepass_max 0 and 0xffffffff, for one and four wavelengths and medium-aware."""
    b = cornell(pkg, lamp, glass_body=glass)
    rd = pkg.api.render_desc(48, 32, 4, 5, seed=5, hero_wavelengths=hero, medium_aware=medium)
    base, prof = engine.create_scene(b).render(rd)
    assert np.isfinite(base).all() and base[..., 1].sum() > 0
    variants = []
    for name in TUNE_FLAGS:
        t = engine.tuning_default()
        t.flags |= getattr(pkg.api, name)
        variants.append((name, t))
    for v in (0, 0xffffffff):
        t = engine.tuning_default()
        t.light_prepass_max = v
        variants.append(("light_prepass_max=%d" % v, t))
    for name, t in variants:
        film, p = engine.create_scene(b, t).render(rd)
        assert np.array_equal(base.view(np.uint32), film.view(np.uint32)), name
        assert (p.bounce_rays, p.shadow_rays) == (prof.bounce_rays, prof.shadow_rays), name


@pytest.mark.gpu
@pytest.mark.parametrize("lamp,glass,hero", [("quad_xf", True, 1), ("dome", False, 4), ("tri", False, 1)])
def test_gpu_film_equals_the_emulation(engine, emu_ml, pkg, lamp, glass, hero):
    """The same lane code under two compilers: a small mesh-light scene's GPU film equals the host emulation's bit for bit."""
    b = cornell(pkg, lamp, glass_body=glass)
    rd = pkg.api.render_desc(32, 24, 4, 5, seed=9, hero_wavelengths=hero)
    g, _ = engine.create_scene(b).render(rd)
    e, _ = emu_ml.create_scene(b).render(rd)
    assert np.array_equal(g.view(np.uint32), e.view(np.uint32))


@pytest.mark.gpu
def test_gpu_light_sample_entry_equals_the_emulation(engine, emu_ml, pkg):
    """pt_light_sample on the GPU equals ptemu_light_sample (and so the float32 restatement) on a transformed smooth lamp."""
    b = cornell(pkg, "dome")
    rng = np.random.default_rng(4)
    frm = rng.uniform(0, 0.5, (2048, 3)).astype(f32)
    s2 = rng.uniform(0, 1, (2048, 2)).astype(f32)
    g, e = engine.create_scene(b), emu_ml.create_scene(b)
    for entry in (0, 5, len(dome()[1]) - 1):
        dg, pg = g.light_sample(entry, frm, s2)
        de, pe = e.light_sample(entry, frm, s2)
        assert np.array_equal(dg.view(np.uint32), de.view(np.uint32)) and np.array_equal(pg.view(np.uint32), pe.view(np.uint32))


LAMP_OBJ = """# a lamp of two triangles over the Cornell box's light
mtllib lamp.mtl
o lamp
usemtl diffuse_light_cornell
v {a}
v {b}
v {c}
v {d}
f 1 2 3 4
"""


def _scene_toml(pkg, tmp_path, material_name=False):
    p, _ = quad(LAMP_SIZE, LAMP_ORIGIN)
    (tmp_path / "lamp.obj").write_text(LAMP_OBJ.format(**{k: " ".join("%.9g" % x for x in p[i]) for i, k in enumerate("abcd")}))
    (tmp_path / "lamp.mtl").write_text("newmtl diffuse_light_cornell\nKd 1 1 1\n")
    data = os.path.join(pkg.scene_file.DATA_ROOT, "data")
    (tmp_path / "meshes.toml").write_text('[lamp]\nfilename = "%s"\n\n[cornell_box]\nfilename = "%s"\n' % (tmp_path / "lamp.obj", os.path.join(data, "meshes", "cornell_box.obj")))
    lamp_material = 'material_name = "diffuse_light_cornell"\n' if material_name else ""
    text = open(os.path.join(data, "scenes", "cornell_box.toml")).read()
    text = text.replace('meshes = "data/lib_meshes.toml"', 'meshes = "%s"' % (tmp_path / "meshes.toml"))
    rect = text[text.index("[[instances]]\nmaterial_name = \"diffuse_light_cornell\""):text.index("[[instances]]\n# no material_name")]
    text = text.replace(rect, "[[instances]]\n%s[instances.aggregate]\ntype = \"Mesh\"\nname = \"lamp\"\n\n" % lamp_material)
    path = tmp_path / "lamp_scene.toml"
    path.write_text(text)
    return str(path)


@pytest.mark.gpu
def test_gpu_scene_file_with_an_obj_lamp(engine, pkg, tmp_path):
    """A TOML scene whose OBJ lamp names a light material (usemtl) loads through libptscene.so and renders on the engine — the film of the same scene
    built through scene.py, bit for bit; the same lamp with a light material_name on its Mesh aggregate renders too."""
    _scene_file_case(engine, pkg, tmp_path)


def _obj_lamp_builder(pkg):
    b = pkg.scene.cornell_box()
    p, f = quad(LAMP_SIZE, LAMP_ORIGIN)
    b.add_mesh_instance(b.add_mesh(p, f, None, face_materials=b.material("diffuse_light_cornell")))
    b.instances[0] = b.instances.pop()                            # the lamp where the rect stood: instance 0, as in the scene file
    return b


def _scene_file_case(lib, pkg, tmp_path):
    sf = pkg.scene_file.SceneFile(_scene_toml(pkg, tmp_path))
    rd = pkg.api.render_desc(64, 48, 8, 5, seed=11)
    film_f, _ = lib.create_scene(sf).render(rd)
    film_b, _ = lib.create_scene(_obj_lamp_builder(pkg)).render(rd)
    assert film_f[..., 1].sum() > 0 and np.array_equal(film_f.view(np.uint32), film_b.view(np.uint32))
    named = pkg.scene_file.SceneFile(_scene_toml(pkg, tmp_path, material_name=True))
    film_n, _ = lib.create_scene(named).render(rd)
    assert np.isfinite(film_n).all() and film_n[..., 1].sum() > 0


def test_scene_file_with_an_obj_lamp(emu_ml, pkg, tmp_path):
    """(the CPU tier of the GPU test below: the emulation renders the scene file and the builder's scene alike)"""
    _scene_file_case(emu_ml, pkg, tmp_path)
