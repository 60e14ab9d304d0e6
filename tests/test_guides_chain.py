"""Denoiser guides that follow specular chains (include/pt_denoise.h pt_render_guides_chain, DESIGN.md section 13 "Specular chains").  As in
test_denoise.py and test_denoise_albedo.py the definition is exact, so the checks are bit for bit: the CPU tier compares the host emulation (the
rules header compiled for the host) with a numpy restatement that walks the chains itself from the probes; the GPU tier compares the engine with
the emulation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emulation
import test_denoise as td
import test_denoise_albedo as tda
from test_denoise import F, PT_ERR_INVALID_ARGUMENT, PT_OK, bits_equal, f32p, u32p

i32p = C.POINTER(C.c_int32)
CHAIN_MAX = 16
DEFAULT_ALPHA_MAX = F(0.01)
KIND_LAMBERTIAN, KIND_GGX, KIND_PASSTHROUGH = 0, 1, 4
TAG_MATERIAL, TAG_LIGHT, TAG_CAMERA = 0, 1, 2
# how a sample ended (np_chain's diagnostics)
END_MISS, END_TERMINAL, END_CAP, END_NOT_FINITE = 0, 1, 2, 3


@pytest.fixture(scope="session")
def emu_ch(pkg):
    """test_denoise_albedo.py's emulation library plus ptemu_guides_chain.cpp: a library of its own."""
    return emulation.load(pkg, "guides_chain")


# ------------------------------------------------------------------------------------------------ numpy restatement of the one-vertex rule
def v3(x, y, z):
    return np.stack([np.asarray(x, F), np.asarray(y, F), np.asarray(z, F)], -1)


def np_dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def np_scale(a, s):
    return a * np.asarray(s, F)[..., None]


def np_normalize(a):
    return a / np.sqrt(np_dot(a, a))[..., None]


def np_frame(n):
    """frame_from_normal (Duff et al.): the sign is the normal's sign BIT."""
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    sign = np.where(np.signbit(nz), F(-1.0), F(1.0)).astype(F)
    a = F(-1.0) / (sign + nz)
    b = nx * ny * a
    t = v3(F(1.0) + sign * nx * nx * a, sign * b, -sign * nx)
    bt = v3(b, sign + ny * ny * a, -ny)
    return t, bt, n


def np_to_local(fr, v):
    return v3(np_dot(fr[0], v), np_dot(fr[1], v), np_dot(fr[2], v))


def np_to_world(fr, v):
    return (np_scale(fr[0], v[..., 0]) + np_scale(fr[1], v[..., 1])) + np_scale(fr[2], v[..., 2])


def np_reflect(wi, n):
    w = -wi
    return np_normalize(w - np_scale(n, F(2.0) * np_dot(w, n)))


def np_refract(wi, n, eta):
    """refract: (wo, refracted?) — wo is garbage where total internal reflection was reported."""
    cos_i = np_dot(wi, n)
    sin2_i = tda.np_pt_max(F(1.0) - cos_i * cos_i, F(0.0)).astype(F)
    sin2_t = eta * eta * sin2_i
    ok = ~(sin2_t >= F(1.0))
    cos_t = np.sqrt(F(1.0) - sin2_t)
    return np_normalize(np_scale(-wi, eta) + np_scale(n, eta * cos_i - cos_t)), ok


def np_chain_follows(material_id, kind, alpha, alpha_max, vertex, max_chain):
    tag = (material_id >> 16) & 3
    return (tag == TAG_MATERIAL) & ((kind == KIND_PASSTHROUGH) | ((kind == KIND_GGX) & (alpha <= alpha_max))) & (vertex < max_chain)


def np_chain_next(kind, metallic, ei, eo, p, n, d):
    """dn_chain_next for arrays: (finite?, wo, o, d, total internal reflection?)."""
    with np.errstate(all="ignore"):
        fr = np_frame(n)
        wi = np_normalize(np_to_local(fr, -d))
        up = np.broadcast_to(v3(0.0, 0.0, 1.0), wi.shape)
        eta_rel = F(1.0) / np.where(wi[..., 2] < F(0.0), eo / ei, ei / eo).astype(F)
        facing = np.where((wi[..., 2] < F(0.0))[..., None], -up, up).astype(F)   # the normal on wi's side, as the walk's half vector is
        refr, ok = np_refract(wi, facing, eta_rel)
        refl = np_reflect(wi, up)
        dielectric = (kind != KIND_PASSTHROUGH) & (metallic == 0)
        wo = np.where((kind == KIND_PASSTHROUGH)[..., None], -wi, np.where((dielectric & ok)[..., None], refr, refl)).astype(F)
        side = np.where(wo[..., 2] > F(0.0), F(1.0), F(-1.0)).astype(F)
        o = p + np_scale(np_scale(n, F(0.001)), side)
        dn = np_normalize(np_to_world(fr, wo))
        finite = np.isfinite(o).all(-1) & np.isfinite(dn).all(-1)
    return finite, wo, o.astype(F), dn.astype(F), dielectric & ~ok


def emu_chain_step(emu, normal, point, dirs, material_id, kind, metallic, alpha, ei, eo, vertex, max_chain, alpha_max):
    n = normal.shape[0]
    spec = np.zeros(n, np.int32)
    wo, o, d = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
    fn = emu.lib.ptemu_chain_step
    fn.restype = None
    fn.argtypes = [C.c_size_t, f32p, f32p, f32p, u32p, u32p, u32p, f32p, f32p, f32p, u32p, C.c_uint32, C.c_float, i32p, f32p, f32p, f32p]
    c = np.ascontiguousarray
    fn(n, c(normal, F).ctypes.data_as(f32p), c(point, F).ctypes.data_as(f32p), c(dirs, F).ctypes.data_as(f32p), c(material_id, np.uint32).ctypes.data_as(u32p),
       c(kind, np.uint32).ctypes.data_as(u32p), c(metallic, np.uint32).ctypes.data_as(u32p), c(alpha, F).ctypes.data_as(f32p), c(ei, F).ctypes.data_as(f32p),
       c(eo, F).ctypes.data_as(f32p), c(vertex, np.uint32).ctypes.data_as(u32p), max_chain, float(alpha_max), spec.ctypes.data_as(i32p), wo.ctypes.data_as(f32p),
       o.ctypes.data_as(f32p), d.ctypes.data_as(f32p))
    return spec, wo, o, d


def seeded_step_inputs(n, seed, max_chain, alpha_max):
    """Normals of both z signs (and exact axes), arriving directions from outside and from inside, a share of them grazing; metals, dielectrics of several
    indices, passthrough, Lambertian; alpha just at and just above alpha_max; light and camera tags; vertices up to the cap."""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3)).astype(F)
    nrm = (nrm / np.sqrt((nrm.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(F)
    axes = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [-1, 0, 0]], F)
    pick = rng.random(n) < 0.1
    nrm[pick] = axes[rng.integers(0, 5, int(pick.sum()))]
    # a direction with a chosen cosine against the normal: +-[0.02 .. 1], a fifth of them grazing (|cos| < 2e-3)
    cosv = rng.uniform(0.02, 1.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    graze = rng.random(n) < 0.2
    cosv[graze] = rng.uniform(1e-6, 2e-3, int(graze.sum())) * np.where(rng.random(int(graze.sum())) < 0.5, -1.0, 1.0)
    tang = np.cross(nrm.astype(np.float64), rng.normal(size=(n, 3)))
    tang /= np.sqrt((tang ** 2).sum(-1, keepdims=True))
    dirs = (nrm.astype(np.float64) * cosv[:, None] + tang * np.sqrt(1.0 - cosv ** 2)[:, None]).astype(F)
    point = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    kind = rng.choice(np.array([KIND_GGX, KIND_GGX, KIND_GGX, KIND_PASSTHROUGH, KIND_LAMBERTIAN], np.uint32), n)
    metallic = ((kind == KIND_GGX) & (rng.random(n) < 0.3)).astype(np.uint32)
    above = np.nextafter(F(alpha_max), F(1.0))
    alpha = rng.choice(np.array([0.0004, 0.004, alpha_max, above, 0.02, 0.2], F), n).astype(F)
    ei = rng.choice(np.array([1.33, 1.4557, 2.65, 0.18], F), n).astype(F)
    eo = rng.choice(np.array([1.0, 1.0002772, 1.5], F), n).astype(F)
    tag = rng.choice(np.array([TAG_MATERIAL] * 8 + [TAG_LIGHT, TAG_CAMERA], np.uint32), n)
    material_id = (tag << 16) | rng.integers(0, 40, n).astype(np.uint32)
    vertex = rng.integers(0, max_chain + 1, n).astype(np.uint32)
    return nrm, point, dirs, material_id, kind, metallic, alpha, ei, eo, vertex


# ------------------------------------------------------------------------------------------------ numpy restatement of the whole guide pass
def np_albedo_of_hits(a, lib, sc, builder, rd, h):
    """test_denoise_albedo.np_albedo's rule for the hit records `h`: (1, 1, 1) but for a valid Lambertian hit."""
    lam, wgt = lib.albedo_basis(rd)
    norm = np.zeros(3, F)
    for j in range(tda.J):
        norm = norm + wgt[:, j]
    tex = np.asarray(builder.texture_data, F)
    eps = F(1.1920929e-7)
    n = h.shape[0]
    ak = np.ones((n, 3), F)
    valid = (h["valid"] != 0) & (((h["material"] >> 16) & 3) != a.TAG_CAMERA)
    index = h["material"] & 0xFFFF
    for mi in np.unique(index[valid]):
        m = builder.materials[int(mi)]
        if m.kind != a.MATERIAL_LAMBERTIAN:
            continue
        sel = valid & (index == mi)
        u, v = h["uv"][sel, 0].astype(F), h["uv"][sel, 1].astype(F)
        cu, cv = np.clip(u, F(0.0), F(1.0) - eps), np.clip(v, F(0.0), F(1.0) - eps)
        stack = builder.texstacks[m.texstack]
        energy = np.zeros((int(sel.sum()), tda.J), F)
        for layer in builder.layers[stack.first_layer:stack.first_layer + stack.layer_count]:
            x, y = (cu * F(layer.width)).astype(np.uint32), (cv * F(layer.height)).astype(np.uint32)
            idx = y * np.uint32(layer.width) + x
            c = [sc.curve_eval(layer.curves[q], lam) for q in range(1 if layer.kind == a.TEXTURE1 else 4)]
            if layer.kind == a.TEXTURE1:
                value = c[0][None, :] * tex[layer.data_offset + idx][:, None]
            else:
                t = [tex[layer.data_offset + 4 * idx + q][:, None] for q in range(4)]
                value = (c[0][None, :] * t[0] + c[1][None, :] * t[1]) + (c[2][None, :] * t[2] + c[3][None, :] * t[3])
            energy = energy + value
        rho = td.np_pt_min(energy, F(1.0))
        for ch in range(3):
            s = np.zeros(rho.shape[0], F)
            for j in range(tda.J):
                s = s + rho[:, j] * wgt[ch, j]
            ak[sel, ch] = s / norm[ch] if norm[ch] > 0 else F(1.0)
    return ak


def np_is_metallic(sc, m):
    """pt_scene_host.cpp: the kappa curve summed over 100 steps of the visible range is positive."""
    if m.curve_kappa < 0:
        return False
    step = (F(750.0) - F(380.0)) / F(100.0)
    lam = (F(380.0) + np.arange(100).astype(F) * step).astype(F)
    k = sc.curve_eval(m.curve_kappa, lam)
    s = F(0.0)
    for q in range(100):
        s = F(s + k[q] * step)
    return bool(s > 0)


def np_chain(a, lib, sc, builder, rd, K, max_chain, alpha_max=DEFAULT_ALPHA_MAX, want_albedo=True):
    """The definition from the probes of `sc` (camera_samples, intersect, curve_eval) and the builder's materials: every sample walks its chain here.
    Returns guides, albedo [H,W,4] and per-sample diagnostics: how it ended, at which vertex, the terminal material id, whether it met total internal
    reflection, and the material ids it passed (a list per vertex)."""
    alpha_max = F(alpha_max)
    n = rd.width * rd.height
    px = np.arange(n, dtype=np.uint32)
    nsum, zsum, hits = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, np.uint32)
    asum = np.zeros((n, 3), F)
    diag = []
    metallic_of = {}
    with np.errstate(all="ignore"):
        for k in range(K):
            o, d, lam = sc.camera_samples(rd, px, np.full(n, k, np.uint32))
            active = px.copy()
            length = np.zeros(n, F)
            end, end_vertex, end_material, tir_seen = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, bool)
            passed = []
            rounds = []
            for v in range(max_chain + 1):
                if active.size == 0:
                    break
                rounds.append(int(active.size))
                h = sc.intersect(o, d)
                valid = h["valid"] != 0
                length[active] = np.where(valid, length[active] + h["t"], length[active]).astype(F)
                tag = (h["material"] >> 16) & 3
                index = h["material"] & 0xFFFF
                m = active.size
                kind, alpha, metallic = np.full(m, -1, np.int64), np.zeros(m, F), np.zeros(m, np.uint32)
                ei, eo = np.ones(m, F), np.ones(m, F)
                ordinary = valid & (tag == TAG_MATERIAL)
                for mi in np.unique(index[ordinary]):
                    mat = builder.materials[int(mi)]
                    sel = ordinary & (index == mi)
                    kind[sel] = mat.kind
                    if mat.kind == a.MATERIAL_GGX:
                        alpha[sel] = F(mat.alpha)
                        if F(mat.alpha) <= alpha_max and v < max_chain:   # (material_prepare runs for a vertex the chain follows only)
                            if int(mi) not in metallic_of:
                                metallic_of[int(mi)] = np_is_metallic(sc, mat)
                            metallic[sel] = 1 if metallic_of[int(mi)] else 0
                            ei[sel] = sc.curve_eval(mat.curve_eta, lam[active][sel])
                            eo[sel] = sc.curve_eval(mat.curve_eta_o, lam[active][sel])
                follows = valid & np_chain_follows(h["material"], kind, alpha, alpha_max, v, max_chain)
                finite, _, o2, d2, tir = np_chain_next(kind, metallic, ei, eo, h["point"].astype(F), h["normal"].astype(F), d)
                go = follows & finite
                stop = ~go
                # the samples that end here
                sp = active[stop]
                hv = valid[stop]
                nsum[sp] = np.where(hv[:, None], nsum[sp] + h["normal"][stop], nsum[sp]).astype(F)
                zsum[sp] = np.where(hv, zsum[sp] + length[sp], zsum[sp]).astype(F)
                hits[sp] += hv.astype(np.uint32)
                if want_albedo:
                    asum[sp] = asum[sp] + np_albedo_of_hits(a, lib, sc, builder, rd, h[stop])
                specular_kind = valid & (tag == TAG_MATERIAL) & ((kind == KIND_PASSTHROUGH) | ((kind == KIND_GGX) & (alpha <= alpha_max)))
                end[sp] = np.where(~hv, END_MISS, np.where(follows[stop] & ~finite[stop], END_NOT_FINITE, np.where(specular_kind[stop], END_CAP, END_TERMINAL)))
                end_vertex[sp] = v
                end_material[sp] = np.where(hv, h["material"][stop], np.uint32(0xFFFFFFFF))
                tir_seen[active[go]] |= tir[go]
                mats = np.full(n, 0xFFFFFFFF, np.uint32)
                mats[active[go]] = h["material"][go]
                passed.append(mats)
                active, o, d = active[go], o2[go], d2[go]
            assert active.size == 0
            diag.append(dict(end=end, vertex=end_vertex, material=end_material, tir=tir_seen, passed=passed, rounds=rounds))
        guides = np.zeros((n, 4), F)
        guides[:, :3] = nsum / F(K)
        guides[:, 3] = np.where(hits > 0, zsum / np.maximum(hits, 1).astype(F), F(0.0))
        albedo = np.zeros((n, 4), F)
        albedo[:, :3] = asum / F(K)
    return guides.reshape(rd.height, rd.width, 4), albedo.reshape(rd.height, rd.width, 4), diag


_WALKS = {}


def walk(pkg, emu, name, w, h, K, D, **kw):
    """One emulated and one numpy chain pass per (scene, size, K, D): shared among the tests, never changed."""
    key = (name, w, h, K, D, tuple(sorted(kw.items())))
    if key not in _WALKS:
        builder = getattr(pkg.scene, name)()
        sc = emu.create_scene(builder)
        rd = pkg.api.render_desc(w, h, 10, 4, seed=1, **kw)
        got = sc.render_guides_chain(rd, K, D)
        want = np_chain(pkg.api, emu, sc, builder, rd, K, D)
        _WALKS[key] = (builder, sc, rd, got, want)
    return _WALKS[key]


CPU_CASES = [("cornell_checker_slab", 24, 24, 2, 8), ("cornell_checker_slab", 24, 24, 2, 1), ("cornell_gem", 24, 16, 2, 8), ("cornell_gem", 24, 16, 2, 3),
             ("fog_ball", 16, 16, 1, 8)]


# ------------------------------------------------------------------------------------------------ CPU tier
def test_libraries_export_the_chain_entry(pkg, emu_ch):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    assert hasattr(lib, "pt_render_guides_chain")
    assert hasattr(emu_ch.lib, "ptemu_render_guides_chain") and hasattr(emu_ch.lib, "ptemu_chain_step")
    text = open(os.path.join(td.ROOT, "include", "pt_denoise.h")).read()
    assert "pt_guide_chain_desc" in text and "#define PT_GUIDE_CHAIN_MAX 16" in text
    assert C.sizeof(pkg.api.GuideChainDesc) == 16


def test_one_vertex_rule_equals_the_numpy_restatement(emu_ch):
    """10^4 seeded vertices: whether the chain goes on, and wo and the next ray where the material is one it follows, bit for bit."""
    max_chain, alpha_max = 5, DEFAULT_ALPHA_MAX
    nrm, point, dirs, material_id, kind, metallic, alpha, ei, eo, vertex = seeded_step_inputs(10000, 20261017, max_chain, alpha_max)
    spec, wo, o, d = emu_chain_step(emu_ch, nrm, point, dirs, material_id, kind, metallic, alpha, ei, eo, vertex, max_chain, alpha_max)
    follows = np_chain_follows(material_id, kind.astype(np.int64), alpha, alpha_max, vertex, max_chain)
    finite, wwo, wo_, wd, tir = np_chain_next(kind.astype(np.int64), metallic, ei, eo, point, nrm, dirs)
    assert np.array_equal(spec != 0, follows & finite)
    assert bits_equal(wo[follows], wwo[follows]) and bits_equal(o[follows], wo_[follows]) and bits_equal(d[follows], wd[follows])
    assert np.all(wo[~follows] == 0) and np.all(o[~follows] == 0) and np.all(d[~follows] == 0)
    # the inputs hold what they were built to hold
    wi_z = np_to_local(np_frame(nrm), -dirs)[:, 2]
    ggx = follows & (kind == KIND_GGX)
    assert (ggx & (wi_z < 0)).sum() > 500 and (ggx & (wi_z > 0)).sum() > 500                  # from inside and from outside
    assert (ggx & tir).sum() > 100 and (ggx & (metallic == 0) & ~tir & (wi_z < 0)).sum() > 100   # total internal reflection, and refraction out of the body
    assert (follows & (np.abs(wi_z) < 2e-3)).sum() > 300                                       # grazing
    assert (ggx & (metallic != 0)).sum() > 300 and (follows & (kind == KIND_PASSTHROUGH)).sum() > 300
    above = np.nextafter(alpha_max, F(1.0))
    at = (kind == KIND_GGX) & (alpha == alpha_max) & (vertex < max_chain) & (((material_id >> 16) & 3) == TAG_MATERIAL)
    over = (kind == KIND_GGX) & (alpha == above) & (vertex < max_chain) & (((material_id >> 16) & 3) == TAG_MATERIAL)
    assert at.sum() > 100 and follows[at].all() and over.sum() > 100 and not follows[over].any()
    assert (follows & np.signbit(nrm[:, 2])).sum() > 1000 and (follows & ~np.signbit(nrm[:, 2])).sum() > 1000   # both branches of the frame
    capped = (vertex == max_chain)
    assert capped.sum() > 500 and not follows[capped].any()
    lit = ((material_id >> 16) & 3) != TAG_MATERIAL
    assert lit.sum() > 500 and not follows[lit].any()
    # a metal reflects, a dielectric met from outside refracts to the other side, passthrough goes straight on
    assert np.all(np.sign(wo[ggx & (metallic != 0)][:, 2]) == np.sign(wi_z[ggx & (metallic != 0)]))
    away = ggx & (metallic == 0) & ~tir
    assert np.all(np.sign(wo[away][:, 2]) == -np.sign(wi_z[away]))


def test_one_vertex_rule_ends_the_chain_at_a_ray_that_is_not_finite(emu_ch):
    """An arriving direction of zero length has no local direction: the next ray is NaN and the vertex is terminal."""
    one = lambda *x: np.array([x], F)
    u = lambda x: np.array([x], np.uint32)
    spec, _, _, d = emu_chain_step(emu_ch, one(0, 0, 1), one(0, 0, 0), one(0, 0, 0), u(0), u(KIND_GGX), u(0), np.array([0.0004], F), np.array([1.5], F), np.array([1.0], F),
                                   u(0), 4, DEFAULT_ALPHA_MAX)
    assert spec[0] == 0 and np.isnan(d).all()
    spec, _, _, d = emu_chain_step(emu_ch, one(0, 0, 1), one(0, 0, 0), one(0, 0.6, -0.8), u(0), u(KIND_GGX), u(0), np.array([0.0004], F), np.array([1.5], F), np.array([1.0], F),
                                   u(0), 4, DEFAULT_ALPHA_MAX)
    assert spec[0] == 1 and np.isfinite(d).all()


@pytest.mark.parametrize("name,w,h,K,D", CPU_CASES)
def test_emulated_chain_equals_the_numpy_restatement(emu_ch, pkg, name, w, h, K, D):
    builder, sc, rd, (guides, albedo), (wguides, walbedo, diag) = walk(pkg, emu_ch, name, w, h, K, D)
    assert bits_equal(guides, wguides), "guides: %d values differ" % int((guides.view(np.uint32) != wguides.view(np.uint32)).sum())
    assert bits_equal(albedo, walbedo), "albedo: %d values differ" % int((albedo.view(np.uint32) != walbedo.view(np.uint32)).sum())
    assert np.all(albedo[..., 3] == 0.0)
    followed = sum(int((dg["vertex"] > 0).sum()) for dg in diag)
    assert followed > 0, "no sample of this case follows a chain"
    if name == "cornell_gem":
        # the gem's interior reflections: some samples are still inside at the cap, some met total internal reflection
        assert sum(int((dg["end"] == END_CAP).sum()) for dg in diag) >= 1
        assert all(int(dg["vertex"][dg["end"] == END_CAP].min(initial=D)) == D for dg in diag)
        assert sum(int(dg["tir"].sum()) for dg in diag) >= 1
    if name == "fog_ball":
        ids = [builder.material(m) for m in ("fog_boundary", "haze_boundary")]
        assert any(np.isin(p, ids).any() for dg in diag for p in dg["passed"])
        assert not any((p == builder.material("ggx_glass_murky")).any() for dg in diag for p in dg["passed"])   # alpha 0.2: never followed
    # the engine's loop would have traced these rays per vertex
    rounds = (C.c_uint32 * (CHAIN_MAX + 1))()
    sc.render_guides_chain(rd, K, D)
    emu_ch.lib.ptemu_guides_chain_last_rounds(rounds)
    want = [sum(dg["rounds"][v] for dg in diag if v < len(dg["rounds"])) for v in range(CHAIN_MAX + 1)]
    assert list(rounds) == want


@pytest.mark.parametrize("name,w,h,K", [(c[0], c[1], c[2], c[3]) for c in CPU_CASES if c[4] == 8])
def test_no_chain_is_the_first_hit_guide(emu_ch, pkg, name, w, h, K):
    builder, sc, rd, _, _ = walk(pkg, emu_ch, name, w, h, K, 8)
    guides, albedo = sc.render_guides_chain(rd, K, 0)
    fguides, falbedo = sc.render_guides_albedo(rd, K)
    assert bits_equal(guides, fguides) and bits_equal(albedo, falbedo)
    # ... and the guides do not depend on whether the albedo is asked for
    for D in (0, 8):
        only, none = sc.render_guides_chain(rd, K, D, albedo=False)
        assert none is None and bits_equal(only, sc.render_guides_chain(rd, K, D)[0])


@pytest.mark.parametrize("name", ["cornell_checker", "cornell_box"])
@pytest.mark.parametrize("D", [1, 8, 16])
def test_a_scene_without_specular_materials_gets_the_first_hit_guide(emu_ch, pkg, name, D):
    sc = emu_ch.create_scene(getattr(pkg.scene, name)())
    rd = pkg.api.render_desc(24, 24, 10, 4, seed=1)
    guides, albedo = sc.render_guides_chain(rd, 2, D)
    fguides, falbedo = sc.render_guides_albedo(rd, 2)
    assert bits_equal(guides, fguides) and bits_equal(albedo, falbedo)


def test_alpha_max_decides_what_is_followed(emu_ch, pkg):
    """mixed_primitives: gold (alpha 0.004) is followed by default, rough glass (0.2) is not; an alpha_max of 0.003 follows neither, one of 0.25 both."""
    builder = pkg.scene.mixed_primitives()
    sc = emu_ch.create_scene(builder)
    rd = pkg.api.render_desc(32, 32, 10, 4, seed=1)
    first = sc.render_guides_albedo(rd, 2)
    default = sc.render_guides_chain(rd, 2, 4)
    assert not bits_equal(default[0], first[0])
    assert bits_equal(default[0], sc.render_guides_chain(rd, 2, 4, alpha_max=0.01)[0])
    low = sc.render_guides_chain(rd, 2, 4, alpha_max=0.003)
    assert bits_equal(low[0], first[0]) and bits_equal(low[1], first[1])
    high = sc.render_guides_chain(rd, 2, 4, alpha_max=0.25)
    assert not bits_equal(high[0], default[0])
    want = np_chain(pkg.api, emu_ch, sc, builder, rd, 2, 4, alpha_max=0.25)
    assert bits_equal(high[0], want[0]) and bits_equal(high[1], want[1])


def slab_masks(pkg, emu, w, h, K):
    """On cornell_checker_slab: the pixels whose K first hits all lie on the slab, and the pixels none of whose K samples meets a specular material."""
    builder, sc, rd, _, (_, _, diag) = walk(pkg, emu, "cornell_checker_slab", w, h, K, 8)
    glass = builder.material("ggx_glass")
    all_slab = np.ones(w * h, bool)
    none_specular = np.ones(w * h, bool)
    for dg in diag:
        all_slab &= dg["passed"][0] == glass
        none_specular &= dg["vertex"] == 0
    return all_slab.reshape(h, w), none_specular.reshape(h, w)


def test_the_chain_sees_through_the_slab(emu_ch, pkg):
    w, h, K = 24, 24, 2
    builder, sc, rd, (guides, albedo), _ = walk(pkg, emu_ch, "cornell_checker_slab", w, h, K, 8)
    fguides, falbedo = sc.render_guides_chain(rd, K, 0)
    all_slab, none_specular = slab_masks(pkg, emu_ch, w, h, K)
    assert all_slab.sum() >= 20 and none_specular.sum() >= 20
    assert np.all(falbedo[all_slab][:, :3] == 1.0)
    assert np.all(albedo[all_slab][:, 1] < 1.0)
    assert np.all(guides[all_slab][:, 3] > fguides[all_slab][:, 3])
    assert bits_equal(guides[none_specular], fguides[none_specular]) and bits_equal(albedo[none_specular], falbedo[none_specular])
    # both squares of the checker show through the glass
    y = albedo[all_slab][:, 1]
    assert y.min() < 0.3 and y.max() > 0.6


def _chain_refusals(fn, last_error, api, scene_handle, valid_status):
    """The bad chain descs are refused whatever the scene argument is — the engine needs no device to say so."""
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(api.RenderDesc), C.c_uint32, C.POINTER(api.GuideChainDesc), f32p, f32p]
    rd = api.render_desc(6, 5, 10, 3)
    g, al = np.zeros((5, 6, 4), F), np.zeros((5, 6, 4), F)

    def status(cd, rd_=rd, K=2, guides=g, scene=scene_handle):
        return fn(scene, C.byref(rd_), K, None if cd is None else C.byref(cd), None if guides is None else guides.ctypes.data_as(f32p), al.ctypes.data_as(f32p))

    for cd, word in ((api.GuideChainDesc(17, 0.0), b"max_chain"), (api.GuideChainDesc(0xFFFFFFFF, 0.0), b"max_chain"), (api.GuideChainDesc(8, -0.5), b"alpha_max"),
                     (api.GuideChainDesc(8, float("nan")), b"alpha_max"), (api.GuideChainDesc(8, float("inf")), b"alpha_max"),
                     (api.GuideChainDesc(8, 0.0, (C.c_uint32 * 2)(1, 0)), b"reserved"), (api.GuideChainDesc(8, 0.0, (C.c_uint32 * 2)(0, 7)), b"reserved")):
        assert status(cd) == PT_ERR_INVALID_ARGUMENT, word
        assert word in last_error(), (word, last_error())
    assert status(None) == PT_ERR_INVALID_ARGUMENT
    ok = api.GuideChainDesc(16, 0.0)
    # everything check_guides_args refuses
    assert status(ok, scene=None) == PT_ERR_INVALID_ARGUMENT and b"null" in last_error()
    if scene_handle is not None:
        assert status(ok, K=0) == PT_ERR_INVALID_ARGUMENT and b"guide_samples" in last_error()
        assert status(ok, guides=None) == PT_ERR_INVALID_ARGUMENT
        assert status(ok, rd_=api.render_desc(0, 5, 10, 3)) == PT_ERR_INVALID_ARGUMENT
        assert status(ok, rd_=api.render_desc(6, 5, 10, 3, camera_index=3)) == PT_ERR_INVALID_ARGUMENT
        assert status(ok, rd_=api.render_desc(6, 5, 10, 3, wavelength=(700.0, 400.0))) == PT_ERR_INVALID_ARGUMENT
        assert status(ok, rd_=api.render_desc(1 << 16, 1 << 16, 10, 3)) == PT_ERR_INVALID_ARGUMENT
        assert status(ok) == valid_status
        assert status(api.GuideChainDesc(0, 0.5)) == valid_status


def test_emulation_refuses_bad_chain_arguments(emu_ch, pkg):
    err = emu_ch.lib.ptemu_guides_chain_last_error
    err.restype = C.c_char_p
    sc = emu_ch.create_scene(pkg.scene.cornell_box())
    _chain_refusals(emu_ch.lib.ptemu_render_guides_chain, err, pkg.api, sc.handle, PT_OK)
    with pytest.raises(pkg.api.PtError) as e:
        sc.render_guides_chain(pkg.api.render_desc(6, 5, 10, 3), 2, 17)
    assert "max_chain" in str(e.value)


def test_engine_refuses_bad_chain_arguments_before_it_looks_for_a_device(pkg):
    """Without a device no scene can be made, and a valid desc with no scene is a null argument; a bad desc is named first.  With a device the same
    refusals hold (the GPU tier runs the valid calls)."""
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    _chain_refusals(lib.pt_render_guides_chain, lib.pt_last_error, pkg.api, None, None)


def test_ptcli_refuses_guide_chain_without_denoise(pkg, tmp_path):
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    for args, words in ((["--guide-chain", "8"], ("--guide-chain", "--denoise")), (["--denoise", "--guide-chain", "17"], ("--guide-chain", "16")),
                        (["--denoise", "--guide-alpha-max", "0.1"], ("--guide-alpha-max", "--guide-chain")),
                        (["--denoise", "--guide-chain", "4", "--guide-alpha-max", "-1"], ("--guide-alpha-max",))):
        r = subprocess.run([exe, "--output-dir", str(tmp_path / "refused")] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert r.returncode == 2 and all(wd in r.stderr for wd in words), r.stderr
    assert not (tmp_path / "refused").exists()


# ---- quality
_QUALITY = {}


def quality_setup(pkg, emu):
    """The albedo test's set-up on cornell_checker_slab: 48x48, seed 1, max_bounces 6; one reference of 1000 spp at seed 77, the first-hit and the chain
    guides (K = 4), and the mask: the pixels whose sample-0 chain crosses the slab and ends on the checker."""
    if not _QUALITY:
        builder = pkg.scene.cornell_checker_slab()
        sc = emu.create_scene(builder)
        rd = pkg.api.render_desc(48, 48, 20, td.BOUNCES, seed=1)
        _, _, diag = np_chain(pkg.api, emu, sc, builder, rd, 1, 8, want_albedo=False)
        dg = diag[0]
        crossed = np.zeros(48 * 48, bool)
        for p in dg["passed"]:
            crossed |= p == builder.material("ggx_glass")
        mask = (crossed & (dg["end"] == END_TERMINAL) & (dg["material"] == builder.material("checker"))).reshape(48, 48)
        _QUALITY.update(sc=sc, mask=mask, ref=sc.render(pkg.api.render_desc(48, 48, 1000, td.BOUNCES, seed=77))[0],
                        first=sc.render_guides_albedo(rd, 4), chain=sc.render_guides_chain(rd, 4, 8))
    return _QUALITY


@pytest.mark.parametrize("spp", [20, 40])
def test_chain_guides_protect_the_checker_behind_the_glass(emu_ch, pkg, spp):
    """cornell_checker_slab 48x48, seed 1, max_bounces 6, against 1000 spp of seed 77, the demodulated filter; RMSE over XYZ on the pixels whose sample-0
    chain crosses the slab and ends on the checker.  The same noisy film is filtered twice: with the first-hit guides and albedo (what the filter had
    before) and with the chain's (D = 8).  The condition is the ordering of the two errors; the emulation is deterministic, so there is no margin.
    Measured in the emulation on the 277 masked pixels of 2304 (noisy / first-hit / chain): 20 spp 2.188e-3 / 2.071e-3 / 0.995e-3 (0.480 of first-hit),
    40 spp 1.633e-3 / 1.937e-3 / 0.923e-3 (0.477); the whole film does not move (0.01500 / 0.01498 and 0.01399 / 0.01402): profiles/denoise_quality.json
    "emulation_48_chain", DESIGN.md section 13."""
    q = quality_setup(pkg, emu_ch)
    mask, ref = q["mask"], q["ref"]
    assert mask.sum() >= 0.10 * mask.size, "the mask holds %d of %d pixels" % (int(mask.sum()), mask.size)
    rd = pkg.api.render_desc(48, 48, spp, td.BOUNCES, seed=1)
    film, counts, st, _ = q["sc"].render_adaptive(rd, spp, 0.0, stats=True)
    first = emu_ch.denoise_film(film, counts, st, q["first"][0], albedo=q["first"][1])
    chain = emu_ch.denoise_film(film, counts, st, q["chain"][0], albedo=q["chain"][1])
    e_noisy, e_first, e_chain = (tda.masked_rmse(x, ref, mask) for x in (film, first, chain))
    w_noisy, w_first, w_chain = (td.film_rmse(x, ref) for x in (film, first, chain))
    print("cornell_checker_slab %d spp, %d masked pixels: rmse noisy %.4g, first-hit guides %.4g, chain guides %.4g (%.3f of first-hit); whole film %.4g / %.4g / %.4g"
          % (spp, int(mask.sum()), e_noisy, e_first, e_chain, e_chain / e_first, w_noisy, w_first, w_chain))
    assert e_chain < e_first


# ------------------------------------------------------------------------------------------------ GPU tier
def chain_pair(engine, emu, builder, rd, K, D, **kw):
    gsc, esc = engine.create_scene(builder), emu.create_scene(builder)
    got, want = gsc.render_guides_chain(rd, K, D, **kw), esc.render_guides_chain(rd, K, D, **kw)
    assert bits_equal(got[0], want[0]), "guides: %d values differ" % int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum())
    assert bits_equal(got[1], want[1]), "albedo: %d values differ" % int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum())
    return gsc, esc, got


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,K,D", [("cornell_checker_slab", 48, 48, 4, 8), ("cornell_gem", 48, 32, 2, 8), ("mixed_primitives", 40, 40, 2, 8),
                                          ("panorama_test", 32, 16, 1, 8), ("fog_ball", 32, 32, 2, 8)])
def test_gpu_chain_equals_the_emulation(engine, emu_ch, pkg, name, w, h, K, D):
    builder = getattr(pkg.scene, name)()
    rd = pkg.api.render_desc(w, h, 10, 4, seed=1)
    gsc, esc, got = chain_pair(engine, emu_ch, builder, rd, K, D)
    only, _ = gsc.render_guides_chain(rd, K, D, albedo=False)   # the form without the albedo sum
    assert bits_equal(only, got[0])
    if name in ("cornell_checker_slab", "cornell_gem"):
        assert not bits_equal(got[0], gsc.render_guides_albedo(rd, K)[0])
    if name in ("cornell_checker_slab", "mixed_primitives"):
        # D = 0 is the engine's own first-hit pass
        zero, first = gsc.render_guides_chain(rd, K, 0), gsc.render_guides_albedo(rd, K)
        assert bits_equal(zero[0], first[0]) and bits_equal(zero[1], first[1])


@pytest.mark.gpu
def test_gpu_chain_equals_the_emulation_beyond_one_block_and_twice(engine, emu_ch, pkg):
    """70x45 = 3150 rays: thirteen blocks of 256 lanes, the last one ragged; K = 3, D = 2, other wavelength bounds.  Rays end at different vertices inside a
    wave, so the compaction runs with partly filled waves; a second call gives the same bytes — the order the waves' atomics land in does not show."""
    builder = pkg.scene.cornell_checker_slab()
    rd = pkg.api.render_desc(70, 45, 10, 4, seed=9, wavelength=(400.0, 700.0))
    gsc, esc, got = chain_pair(engine, emu_ch, builder, rd, 3, 2)
    again = gsc.render_guides_chain(rd, 3, 2)
    assert bits_equal(again[0], got[0]) and bits_equal(again[1], got[1])
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


@pytest.mark.gpu
def test_gpu_render_denoised_with_a_chain_equals_the_three_calls(engine, pkg):
    sc = engine.create_scene(pkg.scene.cornell_checker_slab())
    rd = pkg.api.render_desc(64, 64, 20, 5, seed=2)
    film, den, counts, _ = sc.render_denoised(rd, albedo=True, specular_chain=8)
    f2, c2, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
    guides, albedo = sc.render_guides_chain(rd, 4, 8)
    want = engine.denoise_film(f2, c2, st, guides, albedo=albedo)
    assert bits_equal(film, f2) and np.array_equal(counts, c2) and bits_equal(den, want)
    # None is what it was; a chain without the albedo filters with the chain's guides alone
    plain = sc.render_denoised(rd, albedo=True)[1]
    fg, fa = sc.render_guides_albedo(rd, 4)
    assert bits_equal(plain, engine.denoise_film(f2, c2, st, fg, albedo=fa)) and not bits_equal(plain, den)
    assert bits_equal(sc.render_denoised(rd, specular_chain=8)[1], engine.denoise_film(f2, c2, st, guides))


@pytest.mark.gpu
def test_gpu_ptcli_guide_chain(engine, pkg, tmp_path):
    """ptcli --denoise --demodulate-albedo --guide-chain 8 writes the API's film into the <name>_denoised.* files; every other file is byte for byte what a
    run without the flag writes.  The scene is the gem scene of the package's data (moissanite: the chain goes through it)."""
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    text = open(os.path.join(pkg.PACKAGE_DIR, "data", "config_gem_c3.toml")).read()
    text = text.replace("min_samples = 4096", "min_samples = 20").replace("width = 1920", "width = 64").replace("height = 1080", "height = 40")
    text = text.replace("max_bounces = 12", "max_bounces = 5")
    assert "min_samples = 20" in text and "width = 64" in text and "height = 40" in text and "max_bounces = 5" in text
    cfg = tmp_path / "config.toml"
    cfg.write_text(text)
    runs = {}
    for tag, extra in (("albedo", ["--denoise", "--demodulate-albedo"]), ("chain", ["--denoise", "--demodulate-albedo", "--guide-chain", "8"])):
        out = tmp_path / tag
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(out), "--write-film", "--seed", "5"] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = out
    files = sorted(os.listdir(runs["albedo"]))
    assert files == sorted(os.listdir(runs["chain"])) and len(files) == 6
    plain_files = [f for f in files if "_denoised" not in f]
    assert len(plain_files) == 3
    for f in plain_files:
        assert open(runs["albedo"] / f, "rb").read() == open(runs["chain"] / f, "rb").read(), f
    sf = pkg.scene_file
    config = sf.Config(str(cfg))
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    rd = config.render_desc(0, seed=5)
    _, first, _, _ = sc.render_denoised(rd, albedo=True)
    _, chain, _, _ = sc.render_denoised(rd, albedo=True, specular_chain=8)
    npy = [f for f in files if f.endswith("_denoised.npy")][0]
    assert bits_equal(np.load(runs["albedo"] / npy), first)
    assert bits_equal(np.load(runs["chain"] / npy), chain)
    assert not bits_equal(first, chain)
