"""Spectral light groups (include/pt_light_groups_spectral.h): the wavelength bins of every light group from one render, and the re-lamp
of the finished render.

The oracle of a group's bins is the one that judges the group films: group g's bins are the spectral film of the same scene with every emitter outside g
emitting a zero curve (scene.light_groups_room(emit=...)), bit for bit, because the walk never looks at an emission value.  For the same reason a re-lamp has a
yardstick that existing code makes: the room rebuilt with the new curve on the lamp and rendered with the same seed walks the same paths.  The CPU tier checks
the host emulation (tests/host_emulation/ptemu_light_groups_spectral.cpp: ptemu_light_groups.cpp's render loop with the engine's fold text) against the existing
emulated entries, the masked scenes, numpy restatements of the fold, the matrix and the re-lamp, the re-rendered room, every refusal, the header and the command
line; the GPU tier checks the engine against its own existing entries, the masked scenes and the emulation, under pass overlap, and the re-lamp entries."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import emulation
import parity_suite as ps
from test_light_groups import ONLY, ROOM_ENV_GROUP, ROOM_GROUPS, clean_tuning, counters, ptcli, room_rd, same_bits, scaled_c2_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "pt_light_groups_spectral.h")
FRAMES = os.path.join(ROOT, "profiles", "light_groups_spectral_frames.json")
F = np.float32
f32p = C.POINTER(C.c_float)
BINS = (1, 5, 64)
RELAMP_CURVES = ["E10", "blackbody_3000k_x5"]   # (library curves the re-lamp matrices name, added behind the room's own)
RECT = 0                                         # (the rect lamp's group in ROOM_GROUPS: instance 1, with the surfaces that emit nothing)


def fptr(a):
    return a.ctypes.data_as(f32p)


@pytest.fixture(scope="session")
def emu_lgs(pkg):
    """The host emulation (ptemu.cpp) with the group render (ptemu_light_groups.cpp), the development rules (ptemu_spectral_project.cpp) and the spectral group
    render, the matrix and the re-lamp (ptemu_light_groups_spectral.cpp) beside it: a library of its own."""
    return emulation.load(pkg, "light_groups_spectral")


def room(pkg, **kw):
    return pkg.scene.light_groups_room(extra_curves=RELAMP_CURVES, **kw)


def freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def room_renders(lib, pkg):
    """The renders of the room on `lib` (the emulation or the engine), made once and left unchanged: the spectral group render at every bin count, the existing
    group render and spectral renders of the complete scene, and the spectral renders of the three single-emitter scenes."""
    rd = room_rd(pkg)
    sc = lib.create_scene(room(pkg))
    out = {"scene": sc, "lgs": {}, "spectral": {}, "masked": {}}
    out["before"] = sc.render(rd)
    out["lg_before"] = sc.render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    for B in BINS:
        out["lgs"][B] = sc.render_light_groups_spectral(rd, B, ROOM_GROUPS, ROOM_ENV_GROUP)
        freeze(*out["lgs"][B][:4])
    out["resident"] = sc.light_groups_spectral_resident() if lib.prefix == "pt_" else None
    out["lg"] = sc.render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    out["resident_after_plain"] = sc.light_groups_spectral_resident() if lib.prefix == "pt_" else None
    out["after"] = sc.render(rd)
    for B in BINS:
        out["spectral"][B] = sc.render_spectral(rd, B)
    masked = [lib.create_scene(room(pkg, emit=e)) for e in ONLY]
    for B in BINS:
        out["masked"][B] = [m.render_spectral(rd, B) for m in masked]
    return out


@pytest.fixture(scope="session")
def room_emu(pkg, emu_lgs):
    return room_renders(emu_lgs, pkg)


# ------------------------------------------------------------------------------------------------ numpy restatements of the rules
def np_bins(lo, hi, B, lam):
    """x = (lambda - lo) / (span / (float)B); b = x < 0 ? 0 : min((uint32_t)x, B - 1); NaN -> 0.  All f32."""
    lam = np.asarray(lam, F)
    with np.errstate(all="ignore"):
        x = (lam - F(lo)) / ((F(hi) - F(lo)) / F(B))
        inside = (x >= 0) & (x < F(B))
        b = np.where(inside, x, 0).astype(np.uint32)
        return np.where(x >= F(B), np.uint32(B - 1), b).astype(np.uint32)


def np_group_fold(lo, hi, B, energy, u, spp):
    """Group bins [G, B, P] from group energies [G, S, P] and wavelength samples u [S, P]: per group the f32 running sum from 0.0f, in sample order, of the
    energy into the bin of lambda = lo + u * span; then one division by (float)spp."""
    G, S, P = energy.shape
    out = np.zeros((G, B, P), F)
    px = np.arange(P)
    for s in range(S):
        b = np_bins(lo, hi, B, F(lo) + u[s] * (F(hi) - F(lo)))
        for g in range(G):
            out[g, b, px] = out[g, b, px] + energy[g, s]
    return out / F(spp)


def np_relamp(matrix, group_spectral):
    """out[k] = the f32 fold over the planes i = g * B + b ascending of acc = acc + W[k, i] * S_i, from 0.0f; multiply and add are two f32 operations."""
    matrix, gs = np.asarray(matrix, F), np.asarray(group_spectral, F)
    K = matrix.shape[0]
    w, s = matrix.reshape(K, -1), gs.reshape((-1,) + gs.shape[2:])
    out = np.zeros((K,) + gs.shape[2:], F)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = np.zeros(gs.shape[2:], F)
            for i in range(w.shape[1]):
                acc = acc + w[k, i] * s[i]
            out[k] = acc
    return out


def np_sample_lambdas(lo, hi, B, n):
    """lambda[b, j] = lo + ((float)b + ((float)j + 0.5f) / (float)n) * w, w = (hi - lo) / (float)B; all f32."""
    lo, hi = F(lo), F(hi)
    w = (hi - lo) / F(B)
    return (lo + (np.arange(B, dtype=F)[:, None] + (np.arange(n, dtype=F)[None, :] + F(0.5)) / F(n)) * w).astype(F)


def xyz_bar(emu, lam_nm):
    fn = emu.lib.ptemu_xyz_bar
    fn.restype = None
    fn.argtypes = [C.c_size_t, f32p, C.c_int, f32p]
    ang = np.ascontiguousarray(np.asarray(lam_nm, F).ravel() * F(10.0))
    out = np.zeros((ang.size, 3), F)
    fn(ang.size, fptr(ang), 0, fptr(out))
    return out.reshape(np.shape(lam_nm) + (3,))


def np_relamp_matrix(t, q, gain, n):
    """W[k, g, b] = gain[g] * ((m = 0.0f; m = m + t[k, b, j] * q[g, b, j] for j ascending) / (float)n); t [K, B, n], q [G, B, n], all f32."""
    K, G, B = t.shape[0], q.shape[0], t.shape[1]
    out = np.zeros((K, G, B), F)
    with np.errstate(all="ignore"):
        for k in range(K):
            for g in range(G):
                m = np.zeros(B, F)
                for j in range(n):
                    m = m + t[k, :, j] * q[g, :, j]
                out[k, g] = F(gain[g]) * (m / F(n))
    return out


def relamp_case(w, h, G, B, K, seed):
    """Random finite planes and weights of both signs, with zeros."""
    rng = np.random.default_rng(seed)
    gs = rng.uniform(0.05, 4.0, (G, B, h, w)).astype(F)
    gs[rng.random(gs.shape) < 0.4] *= F(-1.0)
    gs[rng.random(gs.shape) < 0.1] = 0.0
    m = rng.uniform(0.01, 2.0, (K, G, B)).astype(F)
    m[rng.random(m.shape) < 0.3] *= F(-1.0)
    m[rng.random(m.shape) < 0.2] = 0.0
    m[K - 1, G - 1, B - 1] = -1.5
    return gs, m


RELAMP_SHAPES_CPU = [(17, 13), (64, 4)]
RELAMP_GROUPS = [1, 3, 8]
RELAMP_K = [1, 3, 9, 16]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def relamp_against_rerender(lib, pkg, B, new_curve, subsamples):
    """The room's rect lamp re-lamped from E5 to `new_curve` on `lib`, and the yardstick: the room rebuilt with that curve on the rect lamp, rendered with the
    same seed.  Returns (relamped [3,H,W], the re-render's group bins developed by the observer rows per group [3,H,W], the observer development of the
    re-render's total bins [3,H,W], the original render, the re-render)."""
    rd = room_rd(pkg)
    b0, b1 = room(pkg), room(pkg, rect_curve=new_curve)
    r0 = lib.create_scene(b0).render_light_groups_spectral(rd, B, ROOM_GROUPS, ROOM_ENV_GROUP)
    r1 = lib.create_scene(b1).render_light_groups_spectral(rd, B, ROOM_GROUPS, ROOM_ENV_GROUP)
    W = b0.light_groups_relamp_matrix(lib, rd, B, "cie", 3, {RECT: ("E5", new_curve)}, subsamples=subsamples)
    R = b0.spectral_response_matrix(lib, rd, B, "cie", subsamples=subsamples)
    keep = np.ascontiguousarray(np.repeat(R[:, None, :], 3, axis=1))
    relamped = lib.light_groups_relamp(r0[3], W)
    return relamped, lib.light_groups_relamp(r1[3], keep), lib.spectral_project(r1[2], R), r0, r1


def recorded():
    return json.load(open(FRAMES))["relamp_against_rerender"]


def general_case(lib, pkg):
    """The relative L2 error of the re-lamped Y plane (rect lamp: E5 -> blackbody_3000k_x5, 16 subsamples) against the development of the re-render's own bins,
    at 8 and 64 bins."""
    err = {}
    for B in (8, 64):
        relamped, _, yard, _, _ = relamp_against_rerender(lib, pkg, B, "blackbody_3000k_x5", 16)
        err[B] = rel_l2(relamped[1], yard[1])
    print("re-lamp E5 -> blackbody_3000k_x5 against the re-render, relative L2 of Y: 8 bins %.6e, 64 bins %.6e" % (err[8], err[64]))
    return err


def check_general_case(err):
    rec = recorded()
    assert err[64] < err[8], err
    assert err[64] < 2.0 * rec["y_rel_l2_bins64"], (err, rec)


def check_exact_case(lib, pkg):
    relamped, yard, _, r0, r1 = relamp_against_rerender(lib, pkg, 8, "E10", 1)
    gs = r0[3]
    live = np.abs(gs[RECT][gs[RECT] != 0])   # (the bins the factor applies to; the sharp disk lamp's far tail reaches the denormals, and its group is kept as it is)
    assert live.size and float(live.min()) > 1e-30 and float(live.max()) < 1e30   # (far from the denormal and the overflow range: a factor of 2 is exact)
    assert float(np.abs(gs).max()) < 1e30
    assert same_bits(r1[3][RECT], F(2.0) * gs[RECT]) and same_bits(r1[3][1], gs[1]) and same_bits(r1[3][2], gs[2])
    assert same_bits(relamped, yard)
    assert not same_bits(r1[0], r0[0]) and float(np.abs(r1[0] - r0[0]).max()) > 1e-3   # (the re-lamped room is another picture: the test is not vacuous)


# ------------------------------------------------------------------------------------------------ CPU tier
def test_emulation_agrees_with_the_existing_entries(room_emu):
    """Film, group films and counters are ptemu_render_light_groups' bit for bit, the total bins the emulation's render_spectral's, whatever the bins."""
    e = room_emu
    film, groups, prof = e["lg"]
    assert same_bits(film, e["before"][0]) and counters(prof) == counters(e["before"][1])
    for B in BINS:
        f, g, s, gs, p = e["lgs"][B]
        assert same_bits(f, film) and same_bits(g, groups) and counters(p) == counters(prof), B
        sf, ss, sp = e["spectral"][B]
        assert same_bits(sf, film) and same_bits(s, ss) and counters(sp) == counters(prof), B
        assert gs.shape == (3, B, 24, 24) and np.isfinite(gs).all()


def test_group_bins_are_the_masked_renders(room_emu):
    """Group g's bins are render_spectral's of the room with only emitter g, bit for bit, at 1, 5 and 64 bins; each group has a positive bin."""
    for B in BINS:
        gs = room_emu["lgs"][B][3]
        for g in range(3):
            mf, ms, mp = room_emu["masked"][B][g]
            assert same_bits(gs[g], ms), (B, g)
            assert same_bits(room_emu["lgs"][B][1][g], mf) and counters(mp) == counters(room_emu["lgs"][B][4]), (B, g)
            assert float(gs[g].max()) > 0.0, (B, g)


def test_empty_group_is_zero_and_one_group_is_the_total(pkg, emu_lgs, room_emu):
    rd = room_rd(pkg)
    sc = emu_lgs.create_scene(room(pkg))
    for B in BINS:
        f, g, s, gs, _ = sc.render_light_groups_spectral(rd, B, (0,) * 6, 0, groups=2)
        assert not gs[1].any() and same_bits(gs[0], s) and same_bits(s, room_emu["lgs"][B][2]) and same_bits(f, room_emu["lg"][0]), B
        f, g, s, gs, _ = sc.render_light_groups_spectral(rd, B, (0,) * 6, 0, groups=1)
        assert gs.shape[0] == 1 and same_bits(gs[0], s) and same_bits(s, room_emu["lgs"][B][2]), B


def test_fold_restated_in_numpy(pkg, emu_lgs, room_emu):
    """The fold from the samples themselves: the emulation hands out every sample's group energies and wavelength sample as the folds read them; the numpy fold
    of those is the group bins, bit for bit."""
    rd = room_rd(pkg)
    a = pkg.api
    fn = emu_lgs.lib.ptemu_light_groups_spectral_samples
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.LightGroupsDesc), f32p, f32p]
    ids = np.asarray(ROOM_GROUPS, np.uint8)
    gd = a.LightGroupsDesc(3, ids.size, ids.ctypes.data_as(C.POINTER(C.c_uint8)), ROOM_ENV_GROUP)
    P = rd.width * rd.height
    energy, u = np.zeros((3, rd.spp, P), F), np.zeros((rd.spp, P), F)
    sc = emu_lgs.create_scene(room(pkg))
    assert fn(sc.handle, C.byref(rd), C.byref(gd), fptr(energy), fptr(u)) == 0
    assert (energy > 0).any() and (u > 0).all() and (u < 1).all()
    for B in BINS:
        want = np_group_fold(rd.wavelength_lo, rd.wavelength_hi, B, energy, u, rd.spp).reshape(3, B, rd.height, rd.width)
        assert same_bits(room_emu["lgs"][B][3], want), B


def test_sums(pkg, emu_lgs, room_emu):
    """The f64 sum over the groups of the group bins within the film bar of the total bins.  A group's observer development against that group's film is
    separated by bin-centre colour matching, far more than the film bar (measured on the emulation at 64 bins: L-inf 2.3e-2, relative 7.2e-1 for the disk lamp's
    group, 2.5e-3 and 3.7e-1 for the rect lamp's), so the comparison that must hold is the exact one: the development of a group's bins is spectral_project of the
    masked render's bins, bit for bit."""
    rd = room_rd(pkg)
    for B in BINS:
        f, g, s, gs, _ = room_emu["lgs"][B]
        d = np.abs(gs.astype(np.float64).sum(axis=0) - s)
        linf, rel = float(d.max()), float((d / np.maximum(np.abs(s.astype(np.float64)), 1e-6)).max())
        print("sum of group bins vs total bins, %d bins: L-inf %.3e relative %.3e" % (B, linf, rel))
        assert linf < ps.FILM_LINF and rel < ps.FILM_REL, (B, linf, rel)
        R = emu_lgs.spectral_observer_matrix(rd, B)
        for k in range(3):
            dev = emu_lgs.spectral_project(gs[k], R)
            dd = np.abs(np.moveaxis(dev.astype(np.float64), 0, -1) - g[k][..., :3])
            print("group %d observer development vs its film, %d bins: L-inf %.3e relative %.3e" %
                  (k, B, float(dd.max()), float((dd / np.maximum(np.abs(g[k][..., :3].astype(np.float64)), 1e-6)).max())))
            assert same_bits(dev, emu_lgs.spectral_project(room_emu["masked"][B][k][1], R)), (B, k)


def test_emulation_passes_keep_the_bits(pkg, emu_lgs, room_emu, monkeypatch):
    """PTEMU_BATCH forces several passes (pixel chunks and sample ranges): the same films and bins, bit for bit."""
    monkeypatch.setenv("PTEMU_BATCH", "2048")
    sc = emu_lgs.create_scene(room(pkg))
    for B in (5, 64):
        f, g, s, gs, p = sc.render_light_groups_spectral(room_rd(pkg), B, ROOM_GROUPS, ROOM_ENV_GROUP)
        w = room_emu["lgs"][B]
        assert same_bits(f, w[0]) and same_bits(g, w[1]) and same_bits(s, w[2]) and same_bits(gs, w[3]) and counters(p) == counters(w[4]), B


def test_matrix_keep_is_the_response_matrix(pkg, emu_lgs):
    """All groups kept, gain 1 (given or not): every group's rows are spectral_response_matrix's bit for bit — CIE rows and curves, behind a filter or not."""
    rd = room_rd(pkg)
    b = room(pkg)
    for n, filt in ((1, None), (16, "flat_78"), (5, "xenon_x5")):
        responses = ("xenon_x5", pkg.api.RESPONSE_CIE_X, pkg.api.RESPONSE_CIE_Y, pkg.api.RESPONSE_CIE_Z, "simple_sky_blue")
        R = b.spectral_response_matrix(emu_lgs, rd, 7, responses, filter=filt, subsamples=n)
        for gain in (None, [1.0] * 4):
            W = b.light_groups_relamp_matrix(emu_lgs, rd, 7, responses, 4, {}, gain=gain, filter=filt, subsamples=n)
            assert W.shape == (5, 4, 7)
            for g in range(4):
                assert same_bits(W[:, g, :], R), (n, filt, g)


@pytest.mark.parametrize("n", [1, 16])
@pytest.mark.parametrize("with_filter", [False, True])
def test_matrix_equals_the_numpy_fold(pkg, emu_lgs, n, with_filter):
    """The matrix against the restated fold over the values of the emulation's curve evaluator and ptemu_xyz_bar: a Flat pair (E5 -> E10), a tabulated pair
    (xenon_x5 -> cornell_light ... a curve with zeros as `old` gives ratio 0 there), a kept group, gains of both signs and zero."""
    rd = room_rd(pkg)
    b = room(pkg)
    pkg.scene.add_library_curves(b, ["cornell_light", "fluorescent_x5"])
    zeros = b.curve_tabulated("lgs_with_zeros", [380.0, 450.0, 500.0, 600.0, 780.0], [0.0, 0.0, 2.0, 0.0, 1.0], mode=pkg.api.INTERP_LINEAR)
    assert zeros == len(b.curves) - 1
    sc = emu_lgs.create_scene(b)
    B, G = 7, 5
    pairs = {0: ("E5", "E10"), 1: ("xenon_x5", "cornell_light"), 3: ("lgs_with_zeros", "blackbody_3000k_x5"), 4: ("fluorescent_x5", "xenon_x5")}
    gain = [1.0, -0.5, 0.0, 3.0, 2.0]
    responses = ("simple_sky_blue", pkg.api.RESPONSE_CIE_X, pkg.api.RESPONSE_CIE_Y, pkg.api.RESPONSE_CIE_Z)
    filt = "flat_78" if with_filter else None
    lam = np_sample_lambdas(rd.wavelength_lo, rd.wavelength_hi, B, n)
    ev = lambda name: sc.curve_eval(b.curve(name), lam.ravel()).reshape(B, n)
    xb = xyz_bar(emu_lgs, lam)
    t = np.stack([ev("simple_sky_blue"), xb[..., 0], xb[..., 1], xb[..., 2]])
    if with_filter:
        t = t * ev(filt)[None]
    q = np.ones((G, B, n), F)
    for g, (o, nw) in pairs.items():
        old, new = ev(o), ev(nw)
        with np.errstate(all="ignore"):
            q[g] = np.where(old > 0, new / old, F(0.0))
    assert (q[3] == 0).any() and (q[3] != 0).any()   # (the curve with zeros is zero at some sample wavelengths and positive at others)
    got = b.light_groups_relamp_matrix(emu_lgs, rd, B, responses, G, pairs, gain=gain, filter=filt, subsamples=n)
    assert same_bits(got, np_relamp_matrix(t, q, gain, n))
    assert not got[:, 2].any() and got[:, 3].any()   # (gain 0 switches a group off; the curve with zeros leaves entries)


@pytest.mark.parametrize("G", RELAMP_GROUPS)
@pytest.mark.parametrize("shape", RELAMP_SHAPES_CPU)
def test_emulation_relamp_is_the_rule(emu_lgs, shape, G):
    """The re-lamp against the numpy fold, bit for bit; where G * bins <= 64, spectral_project of the flattened planes with bins = G * bins gives the same bits."""
    for B in BINS:
        for K in RELAMP_K:
            gs, m = relamp_case(shape[0], shape[1], G, B, K, 1000 * G + 10 * B + K + shape[0])
            got = emu_lgs.light_groups_relamp(gs, m)
            assert same_bits(got, np_relamp(m, gs)), (B, K)
            if G * B <= 64:
                assert same_bits(got, emu_lgs.spectral_project(gs.reshape(G * B, shape[1], shape[0]), m.reshape(K, G * B))), (B, K)


def test_relamp_against_rerender_exact(pkg, emu_lgs):
    """The rect lamp from E5 to a Flat curve of strength 10, CIE responses, one subsample: the ratio is exactly 2, a factor of 2 is exact in every f32 operation,
    and the re-lamped planes are the development of the re-rendered room's group bins bit for bit."""
    check_exact_case(emu_lgs, pkg)


def test_relamp_against_rerender_general(pkg, emu_lgs):
    """The rect lamp from E5 to blackbody_3000k_x5, 16 subsamples, against the development of the re-render's own bins: what separates the two is how far the
    ratio varies inside a bin, so 64 bins are strictly closer than 8.  Recorded on the emulation in profiles/light_groups_spectral_frames.json (relative L2 of
    the Y plane: 8 bins 8.35e-3, 64 bins 4.93e-4); the 64-bin error stays below twice the recorded value."""
    err = general_case(emu_lgs, pkg)
    check_general_case(err)
    rec = recorded()
    assert abs(err[8] - rec["y_rel_l2_bins8"]) < 1e-3 * rec["y_rel_l2_bins8"] and abs(err[64] - rec["y_rel_l2_bins64"]) < 1e-3 * rec["y_rel_l2_bins64"], (err, rec)


def test_refusals(pkg, emu_lgs):
    """Every refusal returns its status and a message of its own."""
    a = pkg.api
    b = room(pkg)
    sc = emu_lgs.create_scene(b)
    ok = dict(width=8, height=8, spp=10, max_bounces=3)
    rd = a.render_desc(**ok)
    cases = [
        ("bins 0", rd, 0, (0,) * 6, 0, 1, 1, "bins must be positive"),
        ("bins 65", rd, 65, (0,) * 6, 0, 1, 1, "at most 64"),
        ("group_count 9", rd, 8, (0,) * 6, 0, 9, 1, "group_count"),
        ("group id", rd, 8, (0, 0, 2, 0, 0, 0), 0, 2, 1, "instance 2"),
        ("environment id", rd, 8, (0,) * 6, 3, 3, 1, "environment_group"),
        ("instance_count", rd, 8, (0,) * 5, 0, 1, 1, "instance_count"),
        ("hero", a.render_desc(hero_wavelengths=4, **ok), 8, (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "one wavelength"),
        ("medium", a.render_desc(medium_aware=True, **ok), 8, (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "medium-aware"),
        ("shard", a.render_desc(shard=(0, 2), **ok), 8, (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "whole film"),
        ("range", a.render_desc(first_sample=0, sample_count=5, **ok), 8, (0,) * 6, 0, 1, a.PT_ERR_UNSUPPORTED, "whole sample range"),
    ]
    seen = set()
    for name, d, B, ids, env, G, status, word in cases:
        with pytest.raises(a.PtError) as e:
            sc.render_light_groups_spectral(d, B, ids, env, groups=G)
        assert e.value.status == status and word in str(e.value), (name, str(e.value))
        seen.add(str(e.value))
    assert len(seen) == len(cases)
    # the matrix
    E5, E10 = b.curve("E5"), b.curve("E10")
    n_curves = len(b.curves)

    def matrix(old, new, gain=None, responses=(a.RESPONSE_CIE_Y,), G=2, **kw):
        return emu_lgs.light_groups_relamp_matrix(rd, 4, responses, G, old, new, gain, b.curves, b.curve_data, **kw)
    mcases = [
        ("gain inf", lambda: matrix([None, E5], [None, E10], [1.0, np.inf]), "the gain of group 1 is not finite"),
        ("gain nan", lambda: matrix([None, E5], [None, E10], [np.nan, 1.0]), "the gain of group 0 is not finite"),
        ("old out of range", lambda: matrix([n_curves, None], [E10, None]), "old_curve of group 0"),
        ("old negative", lambda: matrix([None, -2], [None, E10]), "old_curve of group 1"),
        ("new out of range", lambda: matrix([E5, None], [n_curves, None]), "new_curve of group 0"),
        ("keep new beside an old", lambda: matrix([E5, None], [None, None]), "new_curve is PT_RELAMP_KEEP where old_curve is not"),
        ("non-finite result", lambda: matrix([None, E5], [None, E10], [1.0, 3e38]), "the re-lamp matrix is not finite at response 0, group 1"),
        ("group_count 0", lambda: matrix([], [], G=0), "group_count"),
        ("response", lambda: matrix([None, None], [None, None], responses=(n_curves,)), "response 0"),
        ("subsamples", lambda: matrix([None, None], [None, None], subsamples=17), "subsamples"),
    ]
    seen = set()
    for name, call, word in mcases:
        with pytest.raises(a.PtError) as e:
            call()
        assert e.value.status == 1 and word in str(e.value), (name, str(e.value))
        seen.add(str(e.value))
    assert len(seen) == len(mcases)
    # the re-lamp
    gs, m = relamp_case(4, 4, 2, 3, 2, 1)
    bad = m.copy(); bad[1, 1, 2] = np.inf
    with pytest.raises(a.PtError) as e:
        emu_lgs.light_groups_relamp(gs, bad)
    assert e.value.status == 1 and "re-lamp matrix entry 11 is not finite" in str(e.value)
    with pytest.raises(a.PtError) as e:
        emu_lgs.light_groups_relamp(gs, np.zeros((17, 2, 3), F))
    assert e.value.status == 1 and "at most 16" in str(e.value)
    # the product runs the same checks before it looks for a device: without a scene the first of them is the one that can be seen
    L = pkg.load()
    gd, sd = a.LightGroupsDesc(1, 0, None, 0), a.SpectralDesc(4)
    film = np.zeros((8, 8, 4), F)
    assert L._render_light_groups_spectral(None, C.byref(rd), C.byref(gd), C.byref(sd), fptr(film), None, None, None, None) == 1
    assert L.last_error() == "the scene is null"
    out = np.zeros((2, 4, 4), F)
    assert L._light_groups_relamp(4, 4, 9, 3, 2, fptr(m), fptr(gs), fptr(out)) == 1 and "group_count" in L.last_error()
    assert L._light_groups_relamp(4, 4, 2, 3, 2, fptr(bad), fptr(gs), fptr(out)) == 1 and "is not finite" in L.last_error()
    assert L._light_groups_relamp_resident(None, 2, fptr(m), fptr(out)) == 1 and L.last_error() == "the scene is null"
    with pytest.raises(a.PtError) as e:
        L.light_groups_relamp_matrix(rd, 4, (a.RESPONSE_CIE_Y,), 2, [E5, None], [None, None], None, b.curves, b.curve_data)
    assert "new_curve is PT_RELAMP_KEEP where old_curve is not" in str(e.value)
    assert same_bits(L.light_groups_relamp_matrix(rd, 4, (a.RESPONSE_CIE_Y,), 2, [E5, None], [E10, None], [1.0, 0.5], b.curves, b.curve_data),
                     emu_lgs.light_groups_relamp_matrix(rd, 4, (a.RESPONSE_CIE_Y,), 2, [E5, None], [E10, None], [1.0, 0.5], b.curves, b.curve_data))


def test_header_is_exported_and_the_older_headers_are_untouched(pkg, tmp_path):
    text = open(HEADER).read()
    names = re.findall(r"^pt_status (pt_\w+)\(", text, re.M)
    assert sorted(names) == ["pt_light_groups_relamp", "pt_light_groups_relamp_matrix", "pt_light_groups_relamp_resident", "pt_light_groups_spectral_resident",
                             "pt_render_light_groups_spectral"]
    lib = C.CDLL(pkg.load().path)
    for n in names:
        assert getattr(lib, n) is not None
    assert "#define PT_RELAMP_KEEP (-1)" in text and pkg.api.RELAMP_KEEP == -1
    src = tmp_path / "size.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_light_groups_spectral.h"\nint main(void) { printf("%zu %zu %zu %zu", sizeof(pt_light_groups_desc), '
                   'offsetof(pt_light_groups_desc, instance_group), offsetof(pt_light_groups_desc, environment_group), sizeof(pt_spectral_desc)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off_ids, off_env, ssize = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    D = pkg.api.LightGroupsDesc
    assert (C.sizeof(D), D.instance_group.offset, D.environment_group.offset, C.sizeof(pkg.api.SpectralDesc)) == (size, off_ids, off_env, ssize)


def test_ptcli_flags_while_parsing(pkg):
    """Each forbidden combination exits with status 2 and its own message before any file is read; the existing refusals keep their words; the help and the
    file's head name the flags."""
    exe = ptcli(pkg)
    rl = ["--relamp-groups", "instance", "--relamp-bins", "8"]
    cases = [(rl + extra, "--relamp-groups cannot be combined with " + extra[0]) for extra in (
        ["--adaptive", "0.1"], ["--denoise"], ["--light-groups", "instance"], ["--spectral-bins", "8"], ["--denoise-spectral-bins", "8"], ["--devices", "1"],
        ["--spectral-devices", "1"], ["--hero-wavelengths", "4"])]
    cases += [
        (["--relamp-groups", "face", "--relamp-bins", "8"], "--relamp-groups needs `instance` or `material`"),
        (["--relamp-groups"], "--relamp-groups needs a value"),
        (["--relamp-groups", "instance"], "--relamp-groups needs --relamp-bins"),
        (["--relamp-bins", "8"], "--relamp-bins needs --relamp-groups"),
        (["--relamp-groups", "instance", "--relamp-bins", "65"], "--relamp-bins needs a count in 1..64"),
        (["--relamp-groups", "instance", "--relamp-bins", "0"], "--relamp-bins needs a count in 1..64"),
        (["--relamp", "0:E5"], "--relamp needs --relamp-groups"),
        (["--relamp-gains", "1,2"], "--relamp-gains needs --relamp-groups"),
        (rl + ["--relamp", "E5"], "--relamp needs G:CURVE[,G:CURVE...]"),
        (rl + ["--relamp", "8:E5"], "--relamp needs G:CURVE[,G:CURVE...]"),
        (rl + ["--relamp", "0:"], "--relamp needs G:CURVE[,G:CURVE...]"),
        (rl + ["--relamp", "0:E5,0:E10"], "--relamp names a group twice"),
        (rl + ["--relamp-gains", "1,x"], "--relamp-gains needs finite gains"),
        (rl + ["--relamp-gains", "1,2,3,4,5,6,7,8,9"], "--relamp-gains takes at most 8 gains"),
        (rl + ["--develop-subsamples", "17"], "--develop-subsamples needs a count in 1..16"),
        # the existing flags keep their refusals
        (["--light-groups", "instance", "--spectral-bins", "8"], "--light-groups cannot be combined with --spectral-bins"),
        (["--light-gains", "1,2"], "--light-gains needs --light-groups"),
        (["--develop-subsamples", "4"], "--develop-subsamples needs --develop"),
    ]
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
    flags = "[--relamp-groups instance|material --relamp-bins B [--relamp G:CURVE[,G:CURVE...]] [--relamp-gains g0,g1,...]"
    assert flags in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    assert flags in open(os.path.join(CSRC, "host", "ptcli.cpp")).read().split("#include")[0]


TWO_LIGHTS_OBJ = """mtllib two_lights.mtl
o a
usemtl diffuse_light_cornell
v 0.20 0.20 0.50
v 0.30 0.20 0.50
v 0.30 0.30 0.50
f 1 2 3
usemtl diffuse_light_flat_x5
v 0.20 0.35 0.50
v 0.30 0.35 0.50
v 0.30 0.45 0.50
f 4 5 6
"""


def test_ptcli_dry_run_accepts_the_flags(pkg, tmp_path):
    """A dry run loads the scene, forms the groups, resolves the curves and ends well; what cannot be re-lamped ends it with a message before anything is
    rendered: gains that do not match the groups, an unknown curve, a group that is not there, an HDR-textured environment."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n"]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=str(tmp_path))
    for mode in ("instance", "material"):
        ok = run("--relamp-groups", mode, "--relamp-bins", "8", "--relamp", "0:fluorescent_x5", "--develop-subsamples", "4")
        assert ok.returncode == 0 and re.search(r"light groups: \d+ ", ok.stdout), (ok.stdout, ok.stderr)
    G = int(re.search(r"light groups: (\d+) ", ok.stdout).group(1))
    rl = ["--relamp-groups", "instance", "--relamp-bins", "8"]
    assert run(*rl).returncode == 0
    assert run(*rl, "--relamp-gains", ",".join(["1.5"] * G)).returncode == 0
    bad = run(*rl, "--relamp-gains", ",".join(["1.5"] * (G + 1)))
    assert bad.returncode == 1 and "--relamp-gains needs one gain per group" in bad.stderr, bad.stderr
    bad = run(*rl, "--relamp", "0:no_such_curve")
    assert bad.returncode == 1 and "error: --relamp-groups: --relamp: " in bad.stderr and "no_such_curve" in bad.stderr, bad.stderr
    bad = run(*rl, "--relamp", "%d:E5" % G)
    assert bad.returncode == 1 and ("--relamp names group %d, the scene has %d groups" % (G, G)) in bad.stderr, bad.stderr
    # an environment lit by an HDR texture has no emission curve to replace
    hdr = run("--scene", os.path.join(pkg.PACKAGE_DIR, "data", "scenes", "hdri_small.toml"), *rl)
    assert hdr.returncode == 0 and "the environment last" in hdr.stdout, (hdr.stdout, hdr.stderr)
    env = int(re.search(r"light groups: (\d+) ", hdr.stdout).group(1)) - 1
    bad = run("--scene", os.path.join(pkg.PACKAGE_DIR, "data", "scenes", "hdri_small.toml"), *rl, "--relamp", "%d:E5" % env)
    assert bad.returncode == 1 and "the environment, which an HDR texture lights" in bad.stderr, bad.stderr
    # A mesh whose .mtl names two light materials: the scene file makes one instance per material of a mesh, so each is a group with one curve of its own and can be
    # re-lamped.  (No scene file reaches the refusal of a group whose emitters have different emission curves: with a group per instance or per light material,
    # and one material per instance, every group has one curve.  The refusal guards descriptions whose mesh faces carry several light materials.)
    (tmp_path / "two_lights.obj").write_text(TWO_LIGHTS_OBJ)
    (tmp_path / "two_lights.mtl").write_text("newmtl diffuse_light_cornell\nnewmtl diffuse_light_flat_x5\n")
    (tmp_path / "lib_meshes.toml").write_text('[two_lights]\nfilename = "%s"\n' % (tmp_path / "two_lights.obj"))
    scene = open(os.path.join(pkg.PACKAGE_DIR, "data", "scenes", "cornell_box.toml")).read()
    scene, n = re.subn(r'meshes = "[^"]*"', 'meshes = "%s"' % (tmp_path / "lib_meshes.toml"), scene)
    scene, m = re.subn(r'name = "cornell_box"', 'name = "two_lights"', scene)
    assert (n, m) == (1, 1)
    (tmp_path / "scene.toml").write_text(scene)
    two = run("--scene", str(tmp_path / "scene.toml"), *rl, "--relamp", "0:E5,1:fluorescent_x5,2:blackbody_3000k_x5")
    assert two.returncode == 0 and "light groups: 3 " in two.stdout, (two.stdout, two.stderr)


# ------------------------------------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def room_gpu(engine, pkg):
    return room_renders(engine, pkg)


@pytest.mark.gpu
def test_gpu_agrees_with_the_existing_entries(room_gpu):
    """On one scene handle: film, group films and counters are pt_render_light_groups' bit for bit, the total bins pt_render_spectral's."""
    g = room_gpu
    film, groups, prof = g["lg"]
    for B in BINS:
        f, gf, s, gs, p = g["lgs"][B]
        assert same_bits(f, film) and same_bits(gf, groups) and counters(p) == counters(prof), B
        sf, ss, sp = g["spectral"][B]
        assert same_bits(sf, film) and same_bits(s, ss) and counters(sp) == counters(prof), B
        assert np.isfinite(gs).all()


@pytest.mark.gpu
def test_gpu_group_bins_are_the_masked_renders_and_the_emulations(room_gpu, room_emu):
    for B in BINS:
        f, gf, s, gs, p = room_gpu["lgs"][B]
        for k in range(3):
            assert same_bits(gs[k], room_gpu["masked"][B][k][1]), (B, k)
            assert float(gs[k].max()) > 0.0, (B, k)
        e = room_emu["lgs"][B]
        assert same_bits(f, e[0]) and same_bits(gf, e[1]) and same_bits(s, e[2]) and same_bits(gs, e[3]) and counters(p) == counters(e[4]), B


@pytest.mark.gpu
def test_gpu_eight_groups(engine, pkg, emu_lgs):
    """Six instances dealt over eight groups, the environment in group 7: the emulation's bits at 1, 5 and 64 bins, and the empty groups zero."""
    rd = room_rd(pkg)
    sc, esc = engine.create_scene(room(pkg)), emu_lgs.create_scene(room(pkg))
    ids = (0, 1, 2, 3, 4, 5)
    for B in BINS:
        got = sc.render_light_groups_spectral(rd, B, ids, 7, groups=8)
        want = esc.render_light_groups_spectral(rd, B, ids, 7, groups=8)
        assert all(same_bits(got[i], want[i]) for i in range(4)) and counters(got[4]) == counters(want[4]), B
        assert sc.light_groups_spectral_resident() == (24, 24, 8, B)
        assert not got[3][0].any() and not got[3][6].any() and all(float(got[3][k].max()) > 0.0 for k in (1, 2, 7)), B


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["overlap", "no_overlap", "no_lds"])
def test_gpu_passes_and_tunings_keep_the_bits(engine, pkg, room_gpu, variant):
    """pt_tuning::batch_slots 2048 cuts the render into passes of at most 204 pixels x 10 samples, so both sets of pass buffers are used, every pixel is continued by
    later passes and the cross-pass read-modify-write of k_accumulate_group_bins' LDS columns matters; likewise without the overlap and without LDS staging."""
    flags = {"overlap": 0, "no_overlap": pkg.api.TUNE_NO_PASS_OVERLAP, "no_lds": pkg.api.TUNE_NO_LDS}[variant]
    sc = engine.create_scene(room(pkg), tuning=clean_tuning(engine, pkg, 2048, flags))
    for B in (5, 64):
        f, gf, s, gs, p = sc.render_light_groups_spectral(room_rd(pkg), B, ROOM_GROUPS, ROOM_ENV_GROUP)
        print("passes:", p.kernel_launches[0])
        assert p.kernel_launches[0] >= 7
        w = room_gpu["lgs"][B]
        assert same_bits(f, w[0]) and same_bits(gf, w[1]) and same_bits(s, w[2]) and same_bits(gs, w[3]) and counters(p) == counters(w[4]), B


@pytest.mark.gpu
def test_gpu_other_renders_on_the_same_handle(room_gpu):
    """pt_render and pt_render_light_groups before and after on the same handle give the same bits, and after the plain group render the scene reports no
    resident group bins."""
    g = room_gpu
    assert same_bits(g["before"][0], g["after"][0]) and counters(g["before"][1]) == counters(g["after"][1])
    assert same_bits(g["lg"][0], g["before"][0])
    assert same_bits(g["lg"][0], g["lg_before"][0]) and same_bits(g["lg"][1], g["lg_before"][1]) and counters(g["lg"][2]) == counters(g["lg_before"][2])
    assert g["resident"] == (24, 24, 3, 64) and g["resident_after_plain"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("G", RELAMP_GROUPS)
@pytest.mark.parametrize("shape", [(17, 13), (24, 24)])
def test_gpu_relamp_entries_are_the_rule(engine, pkg, shape, G):
    """pt_light_groups_relamp of random planes, and pt_light_groups_relamp_resident over the bins a render of that size, G and bin count left on the device (the
    room's six instances dealt over the G groups, the environment in the last): the numpy fold, bit for bit, at 1, 5 and 64 bins and K = 1, 3, 9, 16."""
    sc = engine.create_scene(room(pkg))
    for B in BINS:
        _, _, _, gs, _ = sc.render_light_groups_spectral(pkg.api.render_desc(shape[0], shape[1], 10, 4, light_samples=2, seed=G), B, [i % G for i in range(6)], G - 1,
                                                         groups=G, read_groups=False)
        assert sc.light_groups_spectral_resident() == (shape[0], shape[1], G, B) and float(gs[G - 1].max()) > 0.0
        for K in RELAMP_K:
            rs, m = relamp_case(shape[0], shape[1], G, B, K, 1000 * G + 10 * B + K + shape[0])
            assert same_bits(engine.light_groups_relamp(rs, m), np_relamp(m, rs)), (B, K)
            assert same_bits(sc.light_groups_relamp_resident(m), np_relamp(m, gs)), (B, K)


@pytest.mark.gpu
def test_gpu_relamp_resident_follows_the_last_render(engine, pkg, room_gpu):
    """A fresh scene refuses; after a second render of another size, G and bin count the resident re-lamp uses that render's bins; read_bins False leaves the
    device copy usable."""
    fresh = engine.create_scene(room(pkg))
    assert fresh.light_groups_spectral_resident() is None
    with pytest.raises(pkg.api.PtError) as e:
        fresh.light_groups_relamp_resident(np.zeros((1, 3, 5), F))
    assert "no resident group bins" in str(e.value)
    rd = room_rd(pkg)
    _, _, _, gs, _ = fresh.render_light_groups_spectral(rd, 5, ROOM_GROUPS, ROOM_ENV_GROUP)
    _, m = relamp_case(24, 24, 3, 5, 3, 21)
    assert same_bits(fresh.light_groups_relamp_resident(m), np_relamp(m, gs))
    rd2 = pkg.api.render_desc(17, 13, 10, 4, light_samples=1, seed=2)
    _, _, _, gs8, _ = fresh.render_light_groups_spectral(rd2, 7, (0, 1, 2, 3, 4, 5), 7, groups=8)
    assert fresh.light_groups_spectral_resident() == (17, 13, 8, 7) and fresh.spectral_resident() == (17, 13, 7) and fresh.light_groups_resident() == (17, 13, 8)
    _, m8 = relamp_case(17, 13, 8, 7, 9, 22)
    assert same_bits(fresh.light_groups_relamp_resident(m8), np_relamp(m8, gs8))
    f, gf, s, none, _ = fresh.render_light_groups_spectral(rd, 5, ROOM_GROUPS, ROOM_ENV_GROUP, read_bins=False)
    assert s is None and none is None and fresh.light_groups_spectral_resident() == (24, 24, 3, 5)
    assert same_bits(fresh.light_groups_relamp_resident(m), np_relamp(m, room_gpu["lgs"][5][3]))
    R = fresh.library.spectral_observer_matrix(rd, 5)
    assert same_bits(fresh.spectral_project_resident(R), fresh.library.spectral_project(room_gpu["lgs"][5][2], R))


@pytest.mark.gpu
def test_gpu_relamp_against_rerender(engine, pkg):
    """The exact and the general re-lamp tests on the engine, against the same recorded values (engine and emulation agree bit for bit)."""
    check_exact_case(engine, pkg)
    check_general_case(general_case(engine, pkg))


@pytest.mark.gpu
def test_gpu_ptcli_relamp(pkg, tmp_path):
    """ptcli --relamp-groups instance --relamp-bins 8 --relamp 0:CURVE: the usual files byte for byte those of a run without the flags, one spectral EXR per group
    and the re-lamped pair; the re-lamped picture differs from the one made without --relamp."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    rl = ["--relamp-groups", "instance", "--relamp-bins", "8"]
    dry = run("dry", "-n", *rl)
    G = int(re.search(r"light groups: (\d+) ", dry.stdout).group(1))
    plain, lamp, keep = run("plain"), run("lamp", *rl, "--relamp", "0:fluorescent_x5", "--develop-subsamples", "4"), run("keep", *rl)
    assert plain.returncode == 0 and lamp.returncode == 0 and keep.returncode == 0, (plain.stderr, lamp.stderr, keep.stderr)
    usual = sorted(os.listdir(tmp_path / "plain"))
    assert usual and all(open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "lamp" / f, "rb").read() for f in usual)
    extra = sorted(set(os.listdir(tmp_path / "lamp")) - set(usual))
    stem = usual[0].rsplit(".", 1)[0]
    assert extra == sorted(["%s_light%d_spectral.exr" % (stem, g) for g in range(G)] + [stem + "_relamped.exr", stem + "_relamped.png"]), extra
    assert sorted(os.listdir(tmp_path / "keep")) == sorted(os.listdir(tmp_path / "lamp"))
    assert open(tmp_path / "keep" / (stem + "_light0_spectral.exr"), "rb").read() == open(tmp_path / "lamp" / (stem + "_light0_spectral.exr"), "rb").read()
    assert open(tmp_path / "keep" / (stem + "_relamped.exr"), "rb").read() != open(tmp_path / "lamp" / (stem + "_relamped.exr"), "rb").read()
