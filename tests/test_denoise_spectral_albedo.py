"""The per-bin albedo guide and the joint filter that demodulates the wavelength bins by it (pt_render_guides_bin_albedo and pt_denoise_spectral_albedo of
include/pt_spectral.h, DESIGN.md section 14, "Demodulating the bins").  The definition is exact, so every comparison is bit for bit unless a test says
otherwise: the CPU tier compares the host emulation (csrc/pt_denoise_spectral_albedo_rules.h compiled for the host,
tests/host_emulation/ptemu_denoise_spectral_albedo.cpp) with a numpy restatement written here and with the emulations of the entries it extends; the GPU tier
compares the engine with the emulation, the composition with its parts, the demodulated bins with a converged spectral render, and the command line with the
Python calls."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
import test_denoise as td
import test_denoise_albedo as ta
import test_denoise_spectral as ts
from test_denoise import OFF_DEFAULT, bits_equal, np_kwargs, np_variance, synthetic_inputs
from test_spectral import check_spectral_exr, scaled_c2_config
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_NO_DEVICE, PT_ERR_UNSUPPORTED, PT_OK

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
FLOOR = F(1e-3)
u32p, f64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_float)


@pytest.fixture(scope="session")
def emu_ba(pkg):
    """The host emulation with the film denoiser, its albedo form, the chain guides, the joint filter and the per-bin albedo beside it: a library of its own."""
    L = emulation.load(pkg, "denoise_spectral_albedo")
    L.lib.ptemu_denoise_spectral_albedo_last_error.restype = C.c_char_p
    return L


# ------------------------------------------------------------------------------------------------ numpy restatement of the definition
def np_bin_centres(rd, B):
    lo, hi = F(rd.wavelength_lo), F(rd.wavelength_hi)
    w = F((hi - lo) / F(B))
    return (lo + (np.arange(B).astype(F) + F(0.5)) * w).astype(F)


def np_bin_albedo(a, sc, builder, rd, B, K):
    """The definition from the two probes of `sc` (test_denoise_albedo.np_albedo's way): per guide sample the first hit's material; a Lambertian hit's texture
    stack at the B bin centres (curve_eval, a nearest-texel lookup of its own into the builder's texture_data) summed over the layers from 0.0f and clamped to 1;
    everything else 1; the f32 mean over K in sample order.  [B,H,W]."""
    lam = np_bin_centres(rd, B)
    n = rd.width * rd.height
    px = np.arange(n, dtype=np.uint32)
    tex = np.asarray(builder.texture_data, F)
    eps = F(1.1920929e-7)
    bsum = np.zeros((n, B), F)
    with np.errstate(all="ignore"):
        for k in range(K):
            o, d, _ = sc.camera_samples(rd, px, np.full(n, k, np.uint32))
            h = sc.intersect(o, d)
            rho = np.ones((n, B), F)
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
                energy = np.zeros((int(sel.sum()), B), F)
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
                rho[sel] = td.np_pt_min(energy, F(1.0))
            bsum = bsum + rho
        out = bsum / F(K)
    return np.ascontiguousarray(out.T.reshape(B, rd.height, rd.width), F)


def np_dead(film, counts, stats, spectral, albedo=None, bin_albedo=None):
    """The pixels the definition calls dead: the film, the variance or a bin not finite, before or after its division."""
    film, s = np.asarray(film, F), np.asarray(spectral, F)
    with np.errstate(all="ignore"):
        d = ta.np_pt_max(np.asarray(albedo, F)[..., :3], FLOOR) if albedo is not None else np.ones(film.shape[:2] + (3,), F)
        db = ta.np_pt_max(np.asarray(bin_albedo, F), FLOOR) if bin_albedo is not None else np.ones(s.shape, F)
        v = np_variance(counts, stats)
        return ~(np.isfinite(film[..., :3]).all(-1) & np.isfinite(v) & np.isfinite(film[..., :3] / d).all(-1) & np.isfinite(v / (d[..., 1] * d[..., 1])) &
                 np.isfinite(s).all(0) & np.isfinite(s / db).all(0))


def np_denoise_spectral_albedo(film, counts, stats, guides, spectral, albedo=None, bin_albedo=None, **kw):
    """pt_denoise_spectral_albedo in np.float32: the film divided by max(albedo, floor) with the variance by the Y factor squared, the bins by max(bin_albedo,
    floor); a pixel dead when the film, the variance or a bin is not finite before or after its division; test_denoise_spectral.np_denoise_spectral's passes on
    what is left; the live pixels multiplied back, the dead ones as they came in.  (film [H,W,4], variance [H,W], bins [B,H,W])"""
    film, s = np.asarray(film, F), np.asarray(spectral, F)
    h, w = counts.shape
    with np.errstate(all="ignore"):
        d = ta.np_pt_max(np.asarray(albedo, F)[..., :3], FLOOR) if albedo is not None else np.ones((h, w, 3), F)
        db = ta.np_pt_max(np.asarray(bin_albedo, F), FLOOR) if bin_albedo is not None else np.ones(s.shape, F)
        v = np_variance(counts, stats)
        c1 = film[..., :3] / d
        v1 = v / (d[..., 1] * d[..., 1])
        q = s / db
        dead = np_dead(film, counts, stats, s, albedo, bin_albedo)
        # (test_denoise_albedo.np_denoise_albedo's hand-over of the demodulated variance: n = 2, S1 = 0, S2 = 2 v' give exactly v'.  A dead pixel gets a NaN bin:
        #  np_denoise_spectral then calls it dead, skips it in every tap and copies it through.)
        c2 = np.full(counts.shape, 2, np.uint32)
        s2 = np.zeros(stats.shape, np.float64)
        s2[..., 1] = 2.0 * v1.astype(np.float64)
        f1 = np.zeros_like(film)
        f1[..., :3] = c1
        f1[dead] = 0.0; s2[dead] = 0.0
        q = q.copy()
        q[:, dead] = np.nan
        out, var, sb = ts.np_denoise_spectral(f1, c2, s2, guides, q, **kw)
        out[..., :3] = out[..., :3] * d
        var = var * (d[..., 1] * d[..., 1])
        sb = sb * db
        out[dead, :3] = film[dead, :3]
        var[dead] = v[dead]
        sb[:, dead] = s[:, dead]
    return out, var.astype(F), sb.astype(F)


# ------------------------------------------------------------------------------------------------ inputs
SCENES = ("cornell_checker", "cornell_checker_rgba", "cornell_box", "hdri_small")
GUIDE_BINS = (1, 7, 16, 64)
_SCENES = {}


def emu_scene(pkg, emu, name):
    """(builder, emulated scene), kept for the session."""
    if name not in _SCENES:
        builder = ta.builder_of(pkg, name)
        _SCENES[name] = (builder, emu.create_scene(builder))
    return _SCENES[name]


def guide_rd(pkg, w=48, h=48, bounds=(380.0, 750.0), seed=1):
    return pkg.api.render_desc(w, h, 10, 4, seed=seed, wavelength=bounds)


def synthetic_bin_albedo(inputs, spectral, where, B, seed):
    """A per-bin albedo for test_denoise_spectral.synthetic_spectral's bins: values in (0.05, 1), ones, exact zeros, values below the floor, values above 1 —
    and, where the film leaves a second live pixel, one bin of 3e36 over an albedo of 0: 3e36 / 1e-3 is beyond f32, the pixel dies of the division alone.
    Returns (spectral with that bin set, bin_albedo [B,H,W], (y, x) of that pixel or None)."""
    film = inputs[0]
    h, w = film.shape[:2]
    rng = np.random.default_rng(seed * 977 + B)
    a = rng.uniform(0.05, 1.0, (B, h, w)).astype(F)
    k = rng.random((B, h, w))
    a[k < 0.1] = 1.0
    a[(k >= 0.1) & (k < 0.15)] = 0.0
    a[(k >= 0.15) & (k < 0.2)] = F(2e-4)
    a[(k >= 0.2) & (k < 0.25)] = F(1e-3)
    a[(k >= 0.25) & (k < 0.3)] = rng.uniform(1.0, 3.0, int(((k >= 0.25) & (k < 0.3)).sum())).astype(F)
    spectral = spectral.copy()
    live = np.isfinite(film[..., :3]).all(-1) & np.isfinite(np_variance(inputs[1], inputs[2])) & np.isfinite(spectral).all(0)
    ys, xs = np.nonzero(live)
    division = None
    if ys.size >= 2:
        order = np.argsort(np.abs(ys - h // 2) + np.abs(xs - w // 2), kind="stable")
        division = (int(ys[order[1]]), int(xs[order[1]]))
        assert division != where
        spectral[B - 1, division[0], division[1]] = F(3e36)
        a[B - 1, division[0], division[1]] = 0.0
    return spectral, a, division


def synthetic_case(w, h, seed, B):
    """(inputs, spectral, albedo [H,W,4], bin_albedo [B,H,W], (pixel dead through a bin, pixel dead through the division))"""
    inputs = synthetic_inputs(w, h, seed)
    spectral, where = ts.synthetic_spectral(inputs, B, seed)
    spectral, bin_albedo, division = synthetic_bin_albedo(inputs, spectral, where, B, seed)
    return inputs, spectral, ta.seeded_albedo(w, h, seed + 100), bin_albedo, (where, division)


def call(lib, inputs, spectral, albedo, bin_albedo, **kw):
    """(film, variance, bins)"""
    out, out_spectral, var = lib.denoise_spectral_albedo(*inputs, spectral, albedo, bin_albedo, variance=True, **kw)
    return out, var, out_spectral


def differing(a, b):
    return int((np.ascontiguousarray(a, F).view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32)).sum())


# ------------------------------------------------------------------------------------------------ CPU tier: the guide
@pytest.mark.parametrize("name", SCENES)
def test_emulated_bin_albedo_equals_the_numpy_restatement(emu_ba, pkg, name):
    """48x48, K = 4 and K = 1, B in (1, 7, 16, 64), and a second pair of wavelength bounds.  hdri_small's sky pixels are all ones; the rgba checker's planes
    differ from each other, since its albedo varies with wavelength."""
    a = pkg.api
    builder, sc = emu_scene(pkg, emu_ba, name)
    for bounds, cases in (((380.0, 750.0), [(B, K) for B in GUIDE_BINS for K in (4, 1)]), ((400.0, 700.0), [(7, 4)])):
        rd = guide_rd(pkg, bounds=bounds)
        for B, K in cases:
            _, _, got = sc.render_guides_bin_albedo(rd, B, K)
            want = np_bin_albedo(a, sc, builder, rd, B, K)
            assert got.shape == (B, 48, 48)
            assert bits_equal(got, want), (bounds, B, K, "%d values differ" % differing(got, want))
            assert np.all(got >= 0.0) and np.all(got <= 1.0)
            if name == "hdri_small" and K == 4:
                miss = sc.render_guides(rd, K)[..., 3] == 0.0   # (no sample of the pixel hit anything)
                assert miss.any() and np.all(got[:, miss] == F(1.0))
            if name == "cornell_checker_rgba" and B >= 7:
                assert not bits_equal(got[0], got[B - 1]) and not bits_equal(got[0], got[B // 2])
            if name == "cornell_box" and B >= 7:
                assert np.any(got < F(1.0))


def test_sixteen_bins_fold_to_the_xyz_albedo(emu_ba, pkg):
    """The link to the existing guide: at B = 16 the bin centres are pt_albedo_basis' wavelengths bit for bit (asserted first: both are lo + ((float)j + 0.5f) *
    ((hi - lo) / 16), once with (float)bins and once with the literal), so with K = 1 the 16 planes are the rho_j of dn_albedo_lambertian, and folding them with
    the basis weights in its order — sx += rho_j * w[c][j], then sx / norm[c], norm[c] > 0 — gives pt_render_guides_albedo's XYZ albedo bit for bit.  A pixel that
    is not Lambertian holds ones, and sum(1 * w_j) / norm is norm / norm = 1."""
    for name in ("cornell_checker_rgba", "cornell_box", "hdri_small"):
        _, sc = emu_scene(pkg, emu_ba, name)
        for bounds in ((380.0, 750.0), (400.0, 700.0)):
            rd = guide_rd(pkg, bounds=bounds)
            lam, wgt = emu_ba.albedo_basis(rd)
            assert bits_equal(lam, np_bin_centres(rd, 16)) and bits_equal(lam, pkg.load().spectral_bin_centres(rd, 16))
            guides, albedo, planes = sc.render_guides_bin_albedo(rd, 16, 1)
            _, want = sc.render_guides_albedo(rd, 1)
            fold = np.zeros((48, 48, 4), F)
            for ch in range(3):
                norm, s = F(0.0), np.zeros((48, 48), F)
                for j in range(16):
                    norm = F(norm + wgt[ch, j])
                    s = s + planes[j] * wgt[ch, j]
                assert norm > 0
                fold[..., ch] = s / norm
            assert bits_equal(fold, want), (name, bounds, "%d values differ" % differing(fold, want))
            assert bits_equal(albedo, want)


def test_guides_and_xyz_albedo_are_the_existing_entries(emu_ba, pkg):
    """Without a chain the new entry's guides and XYZ albedo are render_guides_albedo's; with one, on the slab, render_guides_chain's.  A scene without specular
    materials gives the first-hit planes for any max_chain; on the slab the chain changes the planes (the checker behind the glass shows in them)."""
    rd = guide_rd(pkg, 32, 32)
    for name in ("cornell_checker", "cornell_box"):
        _, sc = emu_scene(pkg, emu_ba, name)
        g, a, first = sc.render_guides_bin_albedo(rd, 7, 3)
        g0, a0 = sc.render_guides_albedo(rd, 3)
        assert bits_equal(g, g0) and bits_equal(a, a0), name
        for max_chain in (1, 8):
            g2, a2, planes = sc.render_guides_bin_albedo(rd, 7, 3, max_chain=max_chain)
            assert bits_equal(g2, g0) and bits_equal(a2, a0) and bits_equal(planes, first), (name, max_chain)
    builder = pkg.scene.cornell_checker_slab()
    slab = emu_ba.create_scene(builder)
    g, a, chained = slab.render_guides_bin_albedo(rd, 7, 2, max_chain=8)
    g0, a0 = slab.render_guides_chain(rd, 2, 8)
    assert bits_equal(g, g0) and bits_equal(a, a0)
    gf, af, first = slab.render_guides_bin_albedo(rd, 7, 2)
    g1, a1 = slab.render_guides_albedo(rd, 2)
    assert bits_equal(gf, g1) and bits_equal(af, a1)
    assert bits_equal(first, np_bin_albedo(pkg.api, slab, builder, rd, 7, 2))
    assert not bits_equal(chained, first) and not bits_equal(g, gf)
    assert (chained != F(1.0)).sum() > (first != F(1.0)).sum()   # (behind the slab the first hit is glass: ones; the chain ends on the checker)
    # the C entry takes a null albedo_xyzw and a chain desc with max_chain 0
    fn = emu_ba.lib.ptemu_render_guides_bin_albedo
    g3, p3 = np.zeros((32, 32, 4), F), np.zeros((7, 32, 32), F)
    cd = pkg.api.GuideChainDesc(0, 0.0)
    assert fn(slab.handle, C.byref(rd), 2, C.byref(cd), 7, g3.ctypes.data_as(f32p), None, p3.ctypes.data_as(f32p)) == PT_OK
    assert bits_equal(g3, gf) and bits_equal(p3, first)


# ------------------------------------------------------------------------------------------------ CPU tier: the filter
@pytest.mark.parametrize("B", ts.BINS)
@pytest.mark.parametrize("w,h,seed", ts.SIZES)
def test_filter_equals_the_numpy_restatement_on_synthetic_inputs(emu_ba, w, h, seed, B):
    """Film, variance and every bin plane against numpy, with both albedos, with the per-bin albedo alone and with the XYZ albedo alone.  The dead pixels —
    through the film, the statistics, one bin, or the division of one bin alone — come out with their input bits, and nothing they hold spreads."""
    inputs, spectral, albedo, bin_albedo, (where, division) = synthetic_case(w, h, seed, B)
    film = inputs[0]
    assert (bin_albedo < FLOOR).any() or B * w * h < 100
    if (w, h) == (64, 40):
        assert division is not None and (bin_albedo == 0).any() and (bin_albedo == 1).any() and (bin_albedo > 1).any() and ((bin_albedo > 0) & (bin_albedo < FLOOR)).any()
        assert (np.abs(inputs[3][..., :3]).sum(-1) == 0).any()   # (sky pixels)
    for kw in ts.params_for(w, h):
        for alb, balb in ((albedo, bin_albedo), (None, bin_albedo), (albedo, None)):
            got, gvar, gsp = call(emu_ba, inputs, spectral, alb, balb, **kw)
            want, wvar, wsp = np_denoise_spectral_albedo(*inputs, spectral, alb, balb, **np_kwargs(kw))
            tag = (kw, alb is not None, balb is not None)
            assert bits_equal(got, want), (tag, "film: %d values differ" % differing(got, want))
            assert bits_equal(gvar, wvar), tag
            assert bits_equal(gsp, wsp), (tag, "bins: %d values differ" % differing(gsp, wsp))
            dead = np_dead(inputs[0], inputs[1], inputs[2], spectral, alb, balb)
            assert dead[where] and np.isfinite(film[where][:3]).all()
            if division is not None:
                assert np.isfinite(spectral[:, division[0], division[1]]).all() and np.isfinite(film[division][:3]).all()
                assert dead[division] == (balb is not None) or (alb is not None and dead[division])
            assert bits_equal(got[dead][:, :3], film[dead][:, :3]) and bits_equal(gsp[:, dead], spectral[:, dead]), tag
            assert bits_equal(gvar[dead], np_variance(inputs[1], inputs[2])[dead])
            assert (~dead).any() and np.all(np.isfinite(gsp[:, ~dead])) and np.all(np.isfinite(got[~dead]))
            assert np.all(got[..., 3] == 0.0)
        if w * h > 1000 and not np_dead(inputs[0], inputs[1], inputs[2], spectral, None, None)[division]:   # with nothing divided that pixel lives and is filtered
            _, _, gsp = call(emu_ba, inputs, spectral, None, None, **kw)
            assert not bits_equal(gsp[:, division[0], division[1]], spectral[:, division[0], division[1]])


IDENTITY = (37, 53, 12)


def test_no_albedo_and_albedos_of_ones_equal_denoise_spectral(emu_ba):
    """Identity 1: both albedos None, and both all ones (x / 1.0f and x * 1.0f are exact), give ptemu_denoise_spectral's three outputs."""
    w, h, seed = IDENTITY
    inputs = synthetic_inputs(w, h, seed)
    ones = np.ones((h, w, 4), F); ones[..., 3] = 0.0
    for B in (1, 9):
        spectral, _ = ts.synthetic_spectral(inputs, B, seed)
        for kw in ({}, OFF_DEFAULT):
            want = ts.emu_call(emu_ba, inputs, spectral, **kw)
            for alb, balb in ((None, None), (ones, np.ones((B, h, w), F)), (None, np.ones((B, h, w), F)), (ones, None)):
                got = call(emu_ba, inputs, spectral, alb, balb, **kw)
                assert all(bits_equal(g, x) for g, x in zip(got, want)), (B, kw, alb is None, balb is None)


def test_film_and_variance_are_denoise_film_albedos(emu_ba):
    """Identity 2: where no pixel is dead through its bins alone, out_film and out_variance are the denoise_film(albedo=...) emulation's — whatever the per-bin
    albedo is; with the per-bin albedo None the bins are the undemodulated bins filtered with those weights (identity 3: planes that hold the demodulated film
    come out as the demodulated film's planes)."""
    w, h, seed = IDENTITY
    film, counts, stats, guides, albedo = ta.synthetic_with_albedo(w, h, seed)
    inputs = (film, counts, stats, guides)
    spectral, _ = ts.synthetic_spectral(inputs, 9, seed, bin_dead=False)
    with np.errstate(all="ignore"):
        demod = film[..., :3] / ta.np_pt_max(albedo[..., :3], FLOOR)
    film_dead = ~np.isfinite(film[..., :3]).all(-1) | ~np.isfinite(np_variance(counts, stats)) | ~np.isfinite(demod).all(-1)
    spectral = np.where(np.isfinite(spectral), spectral, F(0.25))
    spectral[:, film_dead] = np.nan                                                # (dead either way: no pixel dies through its bins alone)
    bin_albedo = np.random.default_rng(5).uniform(0.05, 1.5, spectral.shape).astype(F)
    for kw in ({}, OFF_DEFAULT):
        want, wvar = emu_ba.denoise_film(*inputs, variance=True, albedo=albedo, **kw)
        for balb in (bin_albedo, None):
            got, gvar, _ = call(emu_ba, inputs, spectral, albedo, balb, **kw)
            assert bits_equal(got, want) and bits_equal(gvar, wvar), (kw, balb is None)
        planes = np.ascontiguousarray(np.moveaxis(np.where(film_dead[..., None], np.nan, demod), -1, 0), F)
        _, _, gsp = call(emu_ba, inputs, planes, albedo, None, **kw)
        with np.errstate(all="ignore"):
            back = gsp * np.moveaxis(ta.np_pt_max(albedo[..., :3], FLOOR), -1, 0)
        assert bits_equal(back[:, ~film_dead], np.moveaxis(want[..., :3], -1, 0)[:, ~film_dead]), kw


def finite_case(B, seed=12):
    """IDENTITY's inputs with finite bins and a per-bin albedo of at least 0.05: no pixel is dead through its bins, and no divisor is the floor."""
    w, h, _ = IDENTITY
    inputs = synthetic_inputs(w, h, seed)
    spectral, _ = ts.synthetic_spectral(inputs, B, seed, bin_dead=False)
    spectral = np.where(np.isfinite(spectral), spectral, F(0.25))
    bin_albedo = np.random.default_rng(seed + B).uniform(0.05, 1.5, spectral.shape).astype(F)
    return inputs, spectral, ta.seeded_albedo(w, h, seed + 100), bin_albedo


def test_each_plane_of_a_wide_call_is_the_one_bin_call(emu_ba):
    """Plane b of a B = 64 call (eight chunks of 8) and of a B = 7 call (the remainder's chunks of 4, 2 and 1) equals the B = 1 call on that plane and its
    albedo plane alone."""
    for B in (64, 7):
        inputs, spectral, albedo, bin_albedo = finite_case(B)
        _, _, wide = call(emu_ba, inputs, spectral, albedo, bin_albedo)
        for b in sorted({0, 3, 4, 5, 6, 7, 8, 31, 56, 62, 63} & set(range(B))):
            _, _, one = call(emu_ba, inputs, spectral[b:b + 1], albedo, bin_albedo[b:b + 1])
            assert bits_equal(wide[b], one[0]), (B, b)


def test_a_power_of_two_in_albedo_and_bins_scales_the_output_exactly(emu_ba):
    """bin_albedo times 4.0f with spectral times 4.0f leaves every s / A as it was (a power of two commutes with the division and with max(A, floor) when no A
    is at the floor), so the passes see the same values and the remodulated output is the unscaled one times 4.0f, bit for bit.  Scaling the bins alone scales
    the output too: the filter is linear in them."""
    inputs, spectral, albedo, bin_albedo = finite_case(9)
    fa, va, a = call(emu_ba, inputs, spectral, albedo, bin_albedo)
    for factor in (F(4.0), F(0.5)):
        fb, vb, b = call(emu_ba, inputs, spectral * factor, albedo, bin_albedo * factor)
        assert bits_equal(fa, fb) and bits_equal(va, vb) and bits_equal(a * factor, b), float(factor)
    _, _, c = call(emu_ba, inputs, spectral * F(2.0), albedo, bin_albedo)
    assert bits_equal(a * F(2.0), c)


# ------------------------------------------------------------------------------------------------ CPU tier: the boundary
def _filter_refusals(fn, last_error, a, valid_status):
    """Every rule of pt_denoise_spectral_albedo's arguments against one library; `valid_status`: what a valid call returns."""
    W, H, B = 6, 5, 3
    film, counts, stats, guides = synthetic_inputs(W, H, 3, dead=False)
    spectral, albedo, balb = np.ones((B, H, W), F), np.full((H, W, 4), 0.5, F), np.full((B, H, W), 0.5, F)
    out, osp, var = np.zeros((H, W, 4), F), np.zeros((B, H, W), F), np.zeros((H, W), F)
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(a.DenoiseDesc), C.c_uint32, f32p, u32p, f64p, f32p, f32p, f32p, f32p, f32p, f32p, f32p]
    P = dict(film=film.ctypes.data_as(f32p), counts=counts.ctypes.data_as(u32p), stats=stats.ctypes.data_as(f64p), guides=guides.ctypes.data_as(f32p),
             albedo=albedo.ctypes.data_as(f32p), spectral=spectral.ctypes.data_as(f32p), balb=balb.ctypes.data_as(f32p), out=out.ctypes.data_as(f32p),
             osp=osp.ctypes.data_as(f32p), var=var.ctypes.data_as(f32p))
    msgs = {}

    def status(key, bins=B, desc=None, null_desc=False, **over):
        p = dict(P); p.update(over)
        d = a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0) if desc is None else desc
        st = fn(None if null_desc else C.byref(d), bins, p["film"], p["counts"], p["stats"], p["guides"], p["albedo"], p["spectral"], p["balb"], p["out"], p["osp"], p["var"])
        if st not in (PT_OK, PT_ERR_NO_DEVICE):
            msgs[key] = last_error().decode()
        return st

    assert status("ok") == valid_status
    assert status("ok", var=None) == valid_status                          # (out_variance may be NULL)
    assert status("ok", albedo=None) == valid_status and status("ok", balb=None) == valid_status and status("ok", albedo=None, balb=None) == valid_status
    assert status("ok", osp=P["spectral"], out=P["film"]) == valid_status  # (the outputs may be the inputs)
    assert status("zero", bins=0) == PT_ERR_INVALID_ARGUMENT
    assert status("many", bins=65) == PT_ERR_INVALID_ARGUMENT
    assert status("spectral", spectral=None) == PT_ERR_INVALID_ARGUMENT
    assert status("out_spectral", osp=None) == PT_ERR_INVALID_ARGUMENT
    assert status("null", null_desc=True) == PT_ERR_INVALID_ARGUMENT
    for name in ("film", "counts", "stats", "guides", "out"):
        assert status("null", **{name: None}) == PT_ERR_INVALID_ARGUMENT, name
    assert status("size", desc=a.DenoiseDesc(0, H, 0, 0.0, 0.0, 0, 0)) == PT_ERR_INVALID_ARGUMENT
    assert status("iterations", desc=a.DenoiseDesc(W, H, 11, 0.0, 0.0, 0, 0)) == PT_ERR_INVALID_ARGUMENT
    assert status("power", desc=a.DenoiseDesc(W, H, 0, 0.0, 0.0, 11, 0)) == PT_ERR_INVALID_ARGUMENT
    assert status("sigma_l", desc=a.DenoiseDesc(W, H, 0, -1.0, 0.0, 0, 0)) == PT_ERR_INVALID_ARGUMENT
    assert status("sigma_z", desc=a.DenoiseDesc(W, H, 0, 0.0, float("nan"), 0, 0)) == PT_ERR_INVALID_ARGUMENT
    r = a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0); r.reserved[0] = 1
    assert status("reserved", desc=r) == PT_ERR_INVALID_ARGUMENT
    c2 = counts.copy(); c2[H - 1, W - 1] = 1
    assert status("count", counts=c2.ctypes.data_as(u32p)) == PT_ERR_INVALID_ARGUMENT
    g2 = guides.copy(); g2[2, 3, 3] = np.nan
    assert status("guide", guides=g2.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf, -0.25):
        a2 = albedo.copy(); a2[1, 2, 1] = bad
        assert status("albedo", albedo=a2.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT, bad
        b2 = balb.copy(); b2[B - 1, H - 1, W - 1] = bad
        assert status("bin_albedo", balb=b2.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT, bad
    z = np.zeros((B, H, W), F)
    assert status("ok", balb=z.ctypes.data_as(f32p)) == valid_status      # (an albedo of exactly 0 is valid: the floor divides)
    assert "ok" not in msgs and all(msgs.values()) and len(set(msgs.values())) == len(msgs), msgs
    assert "bins" in msgs["zero"] and "64" in msgs["many"] and "spectral" in msgs["spectral"] and "out_spectral" in msgs["out_spectral"]
    assert "sample count below 2" in msgs["count"] and "guide" in msgs["guide"] and "iterations" in msgs["iterations"]
    assert "bin_albedo" in msgs["bin_albedo"] and "albedo" in msgs["albedo"] and "bin_albedo" not in msgs["albedo"]


def _guide_refusals(fn, last_error, a, scene, valid_status):
    """Every rule of pt_render_guides_bin_albedo's arguments against one library.  `scene`: a handle, or None — then only the refusals that come before the
    scene is looked at are made, and a call that passes them all is refused for the null scene."""
    W, H, B = 6, 5, 3
    g, alb, planes = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F), np.zeros((B, H, W), F)
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.c_uint32, C.POINTER(a.GuideChainDesc), C.c_uint32, f32p, f32p, f32p]
    msgs = {}

    def status(key, rd=None, samples=2, chain=None, bins=B, guides=g.ctypes.data_as(f32p), albedo=alb.ctypes.data_as(f32p), bin_albedo=planes.ctypes.data_as(f32p), null_rd=False):
        rd = a.render_desc(W, H, 10, 3) if rd is None else rd
        st = fn(scene, None if null_rd else C.byref(rd), samples, None if chain is None else C.byref(chain), bins, guides, albedo, bin_albedo)
        if st != PT_OK:
            msgs[key] = last_error().decode()
        return st

    assert status("zero", bins=0) == PT_ERR_INVALID_ARGUMENT
    assert status("many", bins=65) == PT_ERR_INVALID_ARGUMENT
    assert status("bin_albedo", bin_albedo=None) == PT_ERR_INVALID_ARGUMENT
    assert status("max_chain", chain=a.GuideChainDesc(17, 0.0)) == PT_ERR_INVALID_ARGUMENT
    assert status("alpha", chain=a.GuideChainDesc(4, -1.0)) == PT_ERR_INVALID_ARGUMENT
    cd = a.GuideChainDesc(4, 0.0); cd.reserved[1] = 1
    assert status("reserved", chain=cd) == PT_ERR_INVALID_ARGUMENT
    assert status("null", guides=None) == PT_ERR_INVALID_ARGUMENT
    assert status("null", null_rd=True) == PT_ERR_INVALID_ARGUMENT
    if scene is None:
        assert status("null") == PT_ERR_INVALID_ARGUMENT and status("null", chain=a.GuideChainDesc(4, 0.0)) == PT_ERR_INVALID_ARGUMENT
    else:
        assert status("ok") == valid_status and status("ok", albedo=None) == valid_status and status("ok", chain=a.GuideChainDesc(4, 0.0)) == valid_status
        assert status("ok", chain=a.GuideChainDesc(0, 0.0), bins=64, bin_albedo=np.zeros((64, H, W), F).ctypes.data_as(f32p)) == valid_status
        assert status("samples", samples=0) == PT_ERR_INVALID_ARGUMENT
        assert status("size", rd=a.render_desc(0, H, 10, 3)) == PT_ERR_INVALID_ARGUMENT
        assert status("size", rd=a.render_desc(W, H, 10, 3, camera_index=9)) == PT_ERR_INVALID_ARGUMENT
        assert status("bounds", rd=a.render_desc(W, H, 10, 3, wavelength=(700.0, 400.0))) == PT_ERR_INVALID_ARGUMENT
    assert "ok" not in msgs and all(msgs.values()) and len(set(msgs.values())) == len(msgs), msgs
    assert "bins" in msgs["zero"] and "64" in msgs["many"] and "bin_albedo" in msgs["bin_albedo"] and "max_chain" in msgs["max_chain"] and "alpha_max" in msgs["alpha"]
    return msgs


def test_emulation_refuses_each_bad_argument(emu_ba, pkg):
    _filter_refusals(emu_ba.lib.ptemu_denoise_spectral_albedo, emu_ba.lib.ptemu_denoise_spectral_albedo_last_error, pkg.api, PT_OK)
    _, sc = emu_scene(pkg, emu_ba, "cornell_box")
    with_scene = _guide_refusals(emu_ba.lib.ptemu_render_guides_bin_albedo, emu_ba.lib.ptemu_denoise_spectral_albedo_last_error, pkg.api, sc.handle, PT_OK)
    without = _guide_refusals(emu_ba.lib.ptemu_render_guides_bin_albedo, emu_ba.lib.ptemu_denoise_spectral_albedo_last_error, pkg.api, None, PT_OK)
    assert all(with_scene[k] == without[k] for k in without)
    with pytest.raises(pkg.api.PtError, match="bins: at most 64"):
        sc.render_guides_bin_albedo(guide_rd(pkg, 8, 8), 65)


def test_engine_checks_the_arguments_before_it_looks_for_a_device(emu_ba, pkg):
    """pt_denoise_spectral_albedo takes no scene: its refusals need no GPU, and a valid call without a device is PT_ERR_NO_DEVICE (there is no CPU fallback).
    pt_render_guides_bin_albedo's refusals that come before the scene is read are the emulation's, message for message."""
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_device_count.restype = C.c_uint32
    has_gpu = lib.pt_device_count() > 0
    _filter_refusals(lib.pt_denoise_spectral_albedo, lib.pt_last_error, pkg.api, PT_OK if has_gpu else PT_ERR_NO_DEVICE)
    got = _guide_refusals(lib.pt_render_guides_bin_albedo, lib.pt_last_error, pkg.api, None, PT_OK)
    want = _guide_refusals(emu_ba.lib.ptemu_render_guides_bin_albedo, emu_ba.lib.ptemu_denoise_spectral_albedo_last_error, pkg.api, None, PT_OK)
    assert got == want
    if not has_gpu:
        film, counts, stats, guides = synthetic_inputs(6, 5, 3, dead=False)
        with pytest.raises(pkg.api.PtError, match="no CPU fallback") as e:
            pkg.load().denoise_spectral_albedo(film, counts, stats, guides, np.ones((2, 5, 6), F), np.ones((5, 6, 4), F), np.ones((2, 5, 6), F))
        assert e.value.status == PT_ERR_NO_DEVICE


def test_library_exports_the_entries_and_the_header_stands_alone(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ("pt_render_guides_bin_albedo", "pt_denoise_spectral_albedo"):
        assert hasattr(lib, name), name
    assert not any("bin_albedo" in f or "spectral" in f for f in pkg.api.API_FUNCTIONS)   # (pt_api.h's list: the boundary the oracle shares)
    text = open(os.path.join(ROOT, "include", "pt_spectral.h")).read()
    for name in ("pt_render_guides_bin_albedo", "pt_denoise_spectral_albedo"):
        assert re.search(r"pt_status %s\(" % name, text), name
    src = '#include "pt_spectral.h"\ntypedef pt_status (*guide_fn)(pt_scene*, const pt_render_desc*, uint32_t, const pt_guide_chain_desc*, uint32_t, float*, float*, float*);\n' \
          'typedef pt_status (*filter_fn)(const pt_denoise_desc*, uint32_t, const float*, const uint32_t*, const double*, const float*, const float*, const float*, const float*, ' \
          'float*, float*, float*);\nguide_fn g = pt_render_guides_bin_albedo;\nfilter_fn f = pt_denoise_spectral_albedo;\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t.o"), os.path.join(d, "t.c")])
    e = pkg.load()
    assert e._render_guides_bin_albedo is not None and e._denoise_spectral_albedo is not None


def test_the_old_entries_still_refuse_an_albedo(pkg):
    """denoise_spectral(albedo=...) and render_denoised_spectral(albedo=True) keep refusing with PT_ERR_UNSUPPORTED and "per-bin albedo": the new names are the
    way to demodulate."""
    film, counts, stats, guides = synthetic_inputs(6, 5, 3, dead=False)
    with pytest.raises(pkg.api.PtError, match="per-bin albedo") as e:
        pkg.load().denoise_spectral(film, counts, stats, guides, np.ones((2, 5, 6), F), albedo=np.ones((5, 6, 4), F))
    assert e.value.status == PT_ERR_UNSUPPORTED
    with pytest.raises(pkg.api.PtError, match="per-bin albedo") as e:
        pkg.api.Scene.render_denoised_spectral(None, pkg.api.render_desc(6, 5, 10, 3), 2, albedo=True)   # (refused before the scene is touched)
    assert e.value.status == PT_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ GPU tier
BOUNDS = (380.0, 750.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES + ("cornell_checker_slab",))
def test_gpu_bin_albedo_equals_the_emulation(engine, emu_ba, pkg, name):
    """48x48, K = 4, B = 7 (chunks of 4, 2, 1) and 64 (eight chunks of 8); the slab with max_chain = 8, the others at the first hit.  Guides and XYZ albedo are
    the existing entries' on the engine too."""
    builder = pkg.scene.cornell_checker_slab() if name == "cornell_checker_slab" else ta.builder_of(pkg, name)
    max_chain = 8 if name == "cornell_checker_slab" else 0
    rd = guide_rd(pkg)
    gsc, esc = engine.create_scene(builder), emu_ba.create_scene(builder)
    for B in (7, 64):
        g, a, planes = gsc.render_guides_bin_albedo(rd, B, 4, max_chain=max_chain)
        eg, ea, eplanes = esc.render_guides_bin_albedo(rd, B, 4, max_chain=max_chain)
        assert bits_equal(g, eg) and bits_equal(a, ea), B
        assert bits_equal(planes, eplanes), (B, "%d values differ" % differing(planes, eplanes))
    g0, a0 = gsc.render_guides_chain(rd, 4, 8) if max_chain else gsc.render_guides_albedo(rd, 4)
    assert bits_equal(g, g0) and bits_equal(a, a0)
    if max_chain:
        assert not bits_equal(planes, gsc.render_guides_bin_albedo(rd, 64, 4)[2])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(37, 53), (257, 3)])
def test_gpu_bin_albedo_equals_the_emulation_beyond_one_block(engine, emu_ba, pkg, w, h):
    """37x53 = 1961 and 257x3 = 771 pixels: several blocks of 256 lanes with the last one partly filled; K = 1, 3 and 4; other wavelength bounds; on the rgba
    checker at the first hit and on the slab through its chain."""
    rd = guide_rd(pkg, w, h, bounds=(400.0, 700.0), seed=9)
    for builder, max_chain in ((pkg.scene.cornell_checker(rgba=True), 0), (pkg.scene.cornell_checker_slab(), 8)):
        gsc, esc = engine.create_scene(builder), emu_ba.create_scene(builder)
        for K, B in ((1, 9), (3, 64), (4, 3)):
            got, want = gsc.render_guides_bin_albedo(rd, B, K, max_chain=max_chain), esc.render_guides_bin_albedo(rd, B, K, max_chain=max_chain)
            assert all(bits_equal(x, y) for x, y in zip(got, want)), (max_chain, K, B, differing(got[2], want[2]))


def check_against_emulation(engine, emu, inputs, spectral, albedo, bin_albedo, **kw):
    got, want = call(engine, inputs, spectral, albedo, bin_albedo, **kw), call(emu, inputs, spectral, albedo, bin_albedo, **kw)
    for name, g, x in zip(("film", "variance", "bins"), got, want):
        assert bits_equal(g, x), "%s: %d values differ" % (name, differing(g, x))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", ts.SIZES)
def test_gpu_filter_equals_the_emulation_on_synthetic_inputs(engine, emu_ba, w, h, seed):
    """The CPU tier's inputs, sizes and parameters through the engine at B = 1, 9 and 64, with both albedos and with each alone."""
    for B in (1, 9, 64):
        inputs, spectral, albedo, bin_albedo, _ = synthetic_case(w, h, seed, B)
        for kw in ts.params_for(w, h):
            for alb, balb in ((albedo, bin_albedo), (None, bin_albedo), (albedo, None)):
                check_against_emulation(engine, emu_ba, inputs, spectral, alb, balb, **kw)
    ones = np.ones((h, w, 4), F); ones[..., 3] = 0.0
    want = engine.denoise_spectral(*inputs, spectral, variance=True)
    for alb, balb in ((None, None), (ones, np.ones(spectral.shape, F))):
        got = engine.denoise_spectral_albedo(*inputs, spectral, alb, balb, variance=True)
        assert all(bits_equal(g, x) for g, x in zip(got, want))


_RGBA = {}


def rendered_rgba_checker(engine, pkg, w, h, spp, mx, seed, bounces=td.BOUNCES):
    key = (w, h, spp, mx, seed, bounces)
    if key not in _RGBA:
        sc = engine.create_scene(pkg.scene.cornell_checker(rgba=True))
        rd = pkg.api.render_desc(w, h, spp, bounces, seed=seed, wavelength=BOUNDS)
        film, counts, st, spectral, _ = sc.render_adaptive_spectral(rd, 8, mx, 0.05 if mx > spp else 0.0, step=10, stats=True)
        _RGBA[key] = (sc, rd, (film, counts, st), spectral, sc.render_guides_bin_albedo(rd, 8, 4))
    return _RGBA[key]


@pytest.mark.gpu
def test_gpu_filter_equals_the_emulation_on_the_rendered_rgba_checker(engine, emu_ba, pkg):
    """cornell_checker(rgba=True), 48x48, 20 to 40 spp adaptive, 8 bins: the engine's three calls against the emulation's filter; the film is
    denoise_film(albedo=...)'s; the bins differ from denoise_spectral's."""
    sc, rd, (film, counts, st), spectral, (guides, albedo, bin_albedo) = rendered_rgba_checker(engine, pkg, 48, 48, 20, 40, 3)
    inputs = (film, counts, st, guides)
    got, _, gsp = check_against_emulation(engine, emu_ba, inputs, spectral, albedo, bin_albedo)
    assert bits_equal(got, engine.denoise_film(*inputs, albedo=albedo))
    plain, psp = engine.denoise_spectral(*inputs, spectral)
    assert not bits_equal(gsp, psp) and not bits_equal(got, plain) and not bits_equal(gsp, spectral)


@pytest.mark.gpu
def test_gpu_render_denoised_spectral_with_bin_albedo_equals_the_calls_made_by_hand(engine, pkg):
    a = pkg.api
    rd = a.render_desc(32, 32, 20, 4, seed=2, wavelength=BOUNDS)
    for chain in (0, 8):
        sc = engine.create_scene(pkg.scene.cornell_checker_slab())
        film, den, spectral, den_spectral, counts, prof = sc.render_denoised_spectral(rd, 8, max_samples=40, rel_error=0.05, guide_samples=2, specular_chain=chain, iterations=3,
                                                                                      sigma_luminance=2.0, bin_albedo=True)
        f2, c2, st, s2, _ = sc.render_adaptive_spectral(rd, 8, 40, 0.05, stats=True)
        guides, albedo, bin_albedo = sc.render_guides_bin_albedo(rd, 8, 2, max_chain=chain)
        d2, ds2 = engine.denoise_spectral_albedo(f2, c2, st, guides, s2, albedo, bin_albedo, iterations=3, sigma_luminance=2.0)
        assert bits_equal(film, f2) and np.array_equal(counts, c2) and bits_equal(spectral, s2) and bits_equal(den, d2) and bits_equal(den_spectral, ds2), chain
        assert prof.camera_rays == int(counts.sum()) and not bits_equal(den_spectral, spectral)
        plain = sc.render_denoised_spectral(rd, 8, max_samples=40, rel_error=0.05, guide_samples=2, specular_chain=chain, iterations=3, sigma_luminance=2.0)
        assert not bits_equal(plain[3], den_spectral), chain
        if chain:
            assert bits_equal(guides, sc.render_guides_chain(rd, 2, 8)[0]) and not bits_equal(guides, sc.render_guides(rd, 2))
    with pytest.raises(a.PtError, match="per-bin albedo"):
        sc.render_denoised_spectral(rd, 8, albedo=True)


@pytest.mark.gpu
def test_gpu_demodulated_bins_are_closer_to_a_converged_spectral_render(engine, pkg):
    """cornell_checker(rgba=True), 32x32, 20 spp, 8 bins, defaults, seed 1, against render_spectral at 4000 spp of seed 77: the summed squared error over the
    bins, on the pixels whose sample-0 ray hits the checker (test_denoise_albedo.checker_mask's selection at this film size) and over the whole film.  No
    threshold is set; the three numbers of each region are printed (measured on an MI355X, noisy / denoise_spectral / demodulated: 220 checker pixels 1.070e-2 /
    3.317e-3 / 2.122e-3, the demodulated filter at 0.640 of the plain one; whole film 5.974 / 2.247 / 2.236, 0.995 — the walls, which carry most of the
    film's energy, are untextured).  All three inequalities held.  (tools/denoise_quality.py --size 32 --spp 20 --ref-spp 4000 --spectral-bins 8 --bin-albedo
    writes them into profiles/denoise_quality.json under gpu_32_spectral8_bin_albedo.)"""
    builder = pkg.scene.cornell_checker(rgba=True)
    sc = engine.create_scene(builder)
    rd = pkg.api.render_desc(32, 32, 20, td.BOUNCES, seed=1, wavelength=BOUNDS)
    _, _, spectral, plain, _, _ = sc.render_denoised_spectral(rd, 8)
    _, _, _, demod, _, _ = sc.render_denoised_spectral(rd, 8, bin_albedo=True)
    _, ref, _ = sc.render_spectral(pkg.api.render_desc(32, 32, 4000, td.BOUNCES, seed=77, wavelength=BOUNDS), 8)
    n = 32 * 32
    o, d, _ = sc.camera_samples(rd, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32))
    hit = sc.intersect(o, d)
    mask = ((hit["valid"] != 0) & (hit["material"] == builder.material("checker"))).reshape(32, 32)
    assert 50 < mask.sum() < n
    c_noisy, c_plain, c_demod = (ts.bins_sse(x[:, mask], ref[:, mask]) for x in (spectral, plain, demod))
    w_noisy, w_plain, w_demod = (ts.bins_sse(x, ref) for x in (spectral, plain, demod))
    print("bins, %d checker pixels: summed squared error noisy %.6g, denoise_spectral %.6g, demodulated %.6g (%.3f of the plain filter)" %
          (int(mask.sum()), c_noisy, c_plain, c_demod, c_demod / c_plain))
    print("bins, whole film: summed squared error noisy %.6g, denoise_spectral %.6g, demodulated %.6g (%.3f of the plain filter)" % (w_noisy, w_plain, w_demod, w_demod / w_plain))
    assert c_demod < c_noisy and w_demod < w_noisy
    assert c_demod < c_plain


@pytest.mark.gpu
def test_gpu_ptcli_demodulate_bins(engine, pkg, tmp_path):
    """ptcli --denoise --denoise-spectral-bins 8 --demodulate-bins on test_spectral's scaled C2 config: the file names of the run without the flag; the
    _denoised files are byte for byte those of --denoise --demodulate-albedo; <name>_spectral.exr is unchanged; <name>_denoised_spectral.exr holds
    render_denoised_spectral(bin_albedo=True)'s bins times the factor beside the denoised film's R, G, B; the refused combinations exit non-zero with their
    messages; the help text names the flag."""
    sf = pkg.scene_file
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    spec, bins, film_albedo = (run("spec", "--denoise", "--denoise-spectral-bins", "8"), run("bins", "--denoise", "--denoise-spectral-bins", "8", "--demodulate-bins"),
                               run("albedo", "--denoise", "--demodulate-albedo"))
    for r in (spec, bins, film_albedo):
        assert r.returncode == 0, r.stdout + r.stderr
    assert "beauty_spectral.exr (8 bins)" in bins.stdout and "beauty_denoised_spectral.exr (8 bins)" in bins.stdout
    usual = ["beauty.exr", "beauty.png", "beauty_denoised.exr", "beauty_denoised.png"]
    assert sorted(os.listdir(tmp_path / "bins")) == sorted(os.listdir(tmp_path / "spec")) == sorted(usual + ["beauty_spectral.exr", "beauty_denoised_spectral.exr"])
    for f in usual:
        assert (tmp_path / "bins" / f).read_bytes() == (tmp_path / "albedo" / f).read_bytes(), f
    assert (tmp_path / "bins" / "beauty_spectral.exr").read_bytes() == (tmp_path / "spec" / "beauty_spectral.exr").read_bytes()
    assert (tmp_path / "bins" / "beauty_denoised_spectral.exr").read_bytes() != (tmp_path / "spec" / "beauty_denoised_spectral.exr").read_bytes()
    assert (tmp_path / "bins" / "beauty_denoised.exr").read_bytes() != (tmp_path / "spec" / "beauty_denoised.exr").read_bytes()
    config = sf.Config(str(cfg))
    rd, od = config.render_desc(0, seed=1), config.output_desc(0)
    assert (rd.width, rd.height, rd.spp) == (32, 32, 20) and od.factor == 2.0
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    film, den, spectral, den_spectral, _, _ = sc.render_denoised_spectral(rd, 8, bin_albedo=True)
    centres = engine.spectral_bin_centres(rd, 8)
    _, linear = engine.output_film(den, od.tonemap, od.luminance_only, od.exposure, od.key_value, od.white_point, od.colorspace, od.factor)
    check_spectral_exr(str(tmp_path / "bins" / "beauty_denoised_spectral.exr"), centres, den_spectral * F(od.factor), linear)
    chained = run("chain", "--denoise", "--denoise-spectral-bins", "8", "--demodulate-bins", "--guide-chain", "8")
    assert chained.returncode == 0, chained.stdout + chained.stderr
    _, den8, _, den_spectral8, _, _ = sc.render_denoised_spectral(rd, 8, bin_albedo=True, specular_chain=8)
    _, linear8 = engine.output_film(den8, od.tonemap, od.luminance_only, od.exposure, od.key_value, od.white_point, od.colorspace, od.factor)
    check_spectral_exr(str(tmp_path / "chain" / "beauty_denoised_spectral.exr"), centres, den_spectral8 * F(od.factor), linear8)
    for extra, message in ((["--denoise", "--demodulate-bins"], "--demodulate-bins needs --denoise-spectral-bins"),
                           (["--demodulate-bins"], "--demodulate-bins needs --denoise-spectral-bins"),
                           (["--denoise-spectral-bins", "8", "--demodulate-bins"], "--denoise-spectral-bins needs --denoise"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--demodulate-albedo"], "--denoise-spectral-bins cannot be combined with --demodulate-albedo"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--demodulate-bins", "--demodulate-albedo"],
                            "--denoise-spectral-bins cannot be combined with --demodulate-albedo")):
        r = run("refused", *extra)
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "refused" / "beauty.exr").exists()
    assert "--demodulate-bins" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
