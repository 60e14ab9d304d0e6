"""The albedo guide of the film denoiser and the demodulation of the film by it (include/pt_denoise.h).  As in test_denoise.py
the definition is exact, so the checks are bit for bit: the CPU tier compares the host emulation (the rules header compiled for the host) with a numpy
restatement written operation by operation; the GPU tier compares the engine with the emulation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emulation
import test_denoise as td
from test_denoise import F, PT_ERR_INVALID_ARGUMENT, PT_ERR_NO_DEVICE, PT_OK, bits_equal, f32p, f64p, u32p

J = 16
FLOOR = F(1e-3)
ALBEDO_SCENES = ("cornell_checker", "cornell_checker_rgba", "cornell_box", "cornell_gem", "mixed_primitives", "hdri_small")


def builder_of(pkg, name):
    return pkg.scene.cornell_checker(rgba=True) if name == "cornell_checker_rgba" else getattr(pkg.scene, name)()


@pytest.fixture(scope="session")
def emu_al(pkg):
    """test_denoise.py's emulation library plus ptemu_denoise_albedo.cpp: a library of its own."""
    return emulation.load(pkg, "denoise_albedo")


# ------------------------------------------------------------------------------------------------ numpy restatement of the definition
def np_pt_max(a, b):
    """pt_max: the non-NaN operand if one is NaN."""
    return np.where((a >= b) | (b != b), a, b)


def np_lambda(rd):
    lo, hi = F(rd.wavelength_lo), F(rd.wavelength_hi)
    return (lo + (np.arange(J).astype(F) + F(0.5)) * ((hi - lo) / F(16.0))).astype(F)


def np_xyz_bar64(angstrom):
    """The seven Gaussians of the CIE fit in f64."""
    a = np.asarray(angstrom, np.float64)

    def g(alpha, mu, s1, s2):
        t = (a - mu) / np.where(a < mu, s1, s2)
        return alpha * np.exp(-(t * t) / 2.0)
    return np.stack([g(1.056, 5998.0, 379.0, 310.0) + g(0.362, 4420.0, 160.0, 267.0) + g(-0.065, 5011.0, 204.0, 262.0),
                     g(0.821, 5688.0, 469.0, 405.0) + g(0.286, 5309.0, 163.0, 311.0),
                     g(1.217, 4370.0, 118.0, 360.0) + g(0.681, 4590.0, 260.0, 138.0)])


def np_albedo(a, lib, sc, builder, rd, K):
    """The definition from the two probes of `sc`: per sample the hit's material; a Lambertian hit's texture stack at the 16 wavelengths (curve_eval, a
    nearest-texel lookup of its own into the builder's texture_data), clamped to 1, folded over the library's basis weights; the mean over K.
    `a`: the package's api module."""
    lam, wgt = lib.albedo_basis(rd)
    n = rd.width * rd.height
    px = np.arange(n, dtype=np.uint32)
    norm = np.zeros(3, F)
    for j in range(J):
        norm = norm + wgt[:, j]
    tex = np.asarray(builder.texture_data, F)
    eps = F(1.1920929e-7)
    asum = np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        for k in range(K):
            o, d, _ = sc.camera_samples(rd, px, np.full(n, k, np.uint32))
            h = sc.intersect(o, d)
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
                energy = np.zeros((int(sel.sum()), J), F)
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
                    for j in range(J):
                        s = s + rho[:, j] * wgt[ch, j]
                    ak[sel, ch] = s / norm[ch] if norm[ch] > 0 else F(1.0)
            asum = asum + ak
        out = np.zeros((n, 4), F)
        out[:, :3] = asum / F(K)
    return out.reshape(rd.height, rd.width, 4)


def np_denoise_albedo(film, counts, stats, guides, albedo, **kw):
    """Demodulation, td.np_denoise on the demodulated film with the dead pixels of either side, remodulation; dead pixels as they came in."""
    film, albedo = np.asarray(film, F), np.asarray(albedo, F)
    with np.errstate(all="ignore"):
        d = np_pt_max(albedo[..., :3], FLOOR)
        v = td.np_variance(counts, stats)
        c1 = film[..., :3] / d
        v1 = v / (d[..., 1] * d[..., 1])
        dead = ~(np.isfinite(film[..., :3]).all(-1) & np.isfinite(v) & np.isfinite(c1).all(-1) & np.isfinite(v1))
        # np_denoise takes the variance from counts and stats: the demodulated variance is handed over as statistics of two samples that give it
        # exactly — n = 2, S1 = 0, S2 = 2 v' gives (2 S2 - 0) / (2 * 2 * 1) = v' in f64, and v' is an f32
        c2 = np.full(counts.shape, 2, np.uint32)
        s2 = np.zeros(stats.shape, np.float64)
        s2[..., 1] = 2.0 * v1.astype(np.float64)
        f1 = np.zeros_like(film)
        f1[..., :3] = c1
        f1[dead] = 0.0; s2[dead] = 0.0
        out, var = td.np_denoise(f1, c2, s2, guides, extra_dead=dead, **kw)
        out[..., :3] = out[..., :3] * d
        var = var * (d[..., 1] * d[..., 1])
        out[dead, :3] = film[dead, :3]
        var[dead] = v[dead]
    return out, var.astype(F)


def seeded_albedo(w, h, seed):
    """An albedo plane with values below the floor, exact zeros, ones, bright values — and one tiny enough to push a film value over the f32 range
    (the pixel dies of the division)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w, 4), F)
    a[..., :3] = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    k = rng.random((h, w))
    a[k < 0.1, :3] = 1.0
    a[(k >= 0.1) & (k < 0.15), :3] = 0.0
    a[(k >= 0.15) & (k < 0.2), 1] = F(2e-4)
    a[(k >= 0.2) & (k < 0.25), 0] = F(1e-3)
    a[(k >= 0.25) & (k < 0.3), :3] = rng.uniform(1.0, 3.0, (int(((k >= 0.25) & (k < 0.3)).sum()), 3)).astype(F)
    return a


def synthetic_with_albedo(w, h, seed):
    film, counts, stats, guides = td.synthetic_inputs(w, h, seed)
    albedo = seeded_albedo(w, h, seed + 100)
    y, x = h // 2, w // 2
    film[y, x, :3] = (1.0, F(3e36), 1.0)   # 3e36 / 1e-3 is beyond f32: dead by the division alone
    albedo[y, x, :3] = 0.0
    return film, counts, stats, guides, albedo


def check_albedo_against_numpy(lib, inputs, **kw):
    film, counts, stats, guides, albedo = inputs
    got, gvar = lib.denoise_film(film, counts, stats, guides, variance=True, albedo=albedo, **kw)
    want, wvar = np_denoise_albedo(film, counts, stats, guides, albedo, **td.np_kwargs(kw))
    assert bits_equal(got, want), "film: %d values differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(gvar, wvar), "variance: %d values differ" % int((gvar.view(np.uint32) != wvar.view(np.uint32)).sum())
    assert np.all(got[..., 3] == 0.0)
    return got, gvar


_CHECKER = {}


def checker_inputs(pkg, emu, spp=20):
    """The emulated cornell_checker render of the issue's set-up (48x48, seed 1, max_bounces 6) with guides and albedo of K = 4."""
    if spp not in _CHECKER:
        sc = emu.create_scene(pkg.scene.cornell_checker())
        rd = pkg.api.render_desc(48, 48, spp, td.BOUNCES, seed=1)
        film, counts, st, _ = sc.render_adaptive(rd, spp, 0.0, stats=True)
        guides, albedo = sc.render_guides_albedo(rd, 4)
        _CHECKER[spp] = (film, counts, st, guides, albedo)
    return _CHECKER[spp]


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_the_albedo_entries(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ("pt_albedo_basis", "pt_render_guides_albedo", "pt_denoise_film_albedo"):
        assert hasattr(lib, name), name
    text = open(os.path.join(td.ROOT, "include", "pt_denoise.h")).read()
    assert "#define PT_ALBEDO_WAVELENGTHS 16" in text


@pytest.mark.parametrize("bounds", [(380.0, 750.0), (400.0, 700.0), (555.0, 555.0)])
def test_basis_equals_the_formula_and_the_seven_gaussians(emu_al, pkg, bounds):
    """lambda_j is the f32 formula exactly; the weights are the f64 fit rounded to f32: 1e-6 relative allows for that rounding (6e-8) and for the
    engine's shorter exponential, which the tests of xyz_bar hold to the same f32 bits."""
    rd = pkg.api.render_desc(8, 8, 10, 3, wavelength=bounds)
    lam, w = emu_al.albedo_basis(rd)
    assert bits_equal(lam, np_lambda(rd))
    want = np_xyz_bar64(lam.astype(F) * F(10.0))
    assert np.all(np.abs(w.astype(np.float64) - want) <= 1e-6 * np.abs(want))
    # the engine's own entry needs no device
    plam, pw = pkg.load().albedo_basis(rd)
    assert bits_equal(plam, lam) and bits_equal(pw, w)


@pytest.mark.parametrize("name", ALBEDO_SCENES)
def test_emulated_albedo_equals_the_numpy_restatement(emu_al, pkg, name):
    builder = builder_of(pkg, name)
    sc = emu_al.create_scene(builder)
    rd = pkg.api.render_desc(48, 48, 10, 4, seed=1)
    guides, albedo = sc.render_guides_albedo(rd, 4)
    assert bits_equal(guides, sc.render_guides(rd, 4))
    want = np_albedo(pkg.api, emu_al, sc, builder, rd, 4)
    assert bits_equal(albedo, want), "%d values differ" % int((albedo.view(np.uint32) != want.view(np.uint32)).sum())
    assert np.all(albedo[..., 3] == 0.0) and np.all(albedo[..., :3] > 0.0) and np.all(albedo[..., :3] <= 1.0)
    if name.startswith("cornell_checker"):
        # both squares of the checker are seen, and they differ by about hi / lo
        y = albedo[..., 1]
        assert y.min() < 0.2 and y.max() > 0.6
    if name == "hdri_small":
        sky = np.all(guides[..., :3] == 0.0, -1)
        assert sky.any() and np.all(albedo[sky][:, :3] == 1.0)


def test_emulated_albedo_of_one_sample_and_other_bounds(emu_al, pkg):
    builder = pkg.scene.cornell_checker()
    sc = emu_al.create_scene(builder)
    rd = pkg.api.render_desc(40, 28, 10, 4, seed=5, wavelength=(400.0, 700.0))
    _, albedo = sc.render_guides_albedo(rd, 1)
    assert bits_equal(albedo, np_albedo(pkg.api, emu_al, sc, builder, rd, 1))


def test_filter_equals_the_numpy_restatement_on_the_checker(emu_al, pkg):
    check_albedo_against_numpy(emu_al, checker_inputs(pkg, emu_al))


@pytest.mark.parametrize("w,h,seed,kw", [(37, 23, 61, {}), (70, 9, 62, td.OFF_DEFAULT)])
def test_filter_equals_the_numpy_restatement_on_synthetic_inputs(emu_al, w, h, seed, kw):
    inputs = synthetic_with_albedo(w, h, seed)
    film, albedo = inputs[0], inputs[4]
    assert (albedo[..., :3] < FLOOR).any() and (albedo[..., :3] == 0.0).any() and (albedo[..., :3] == 1.0).any()
    got, gvar = check_albedo_against_numpy(emu_al, inputs, **kw)
    v = td.np_variance(inputs[1], inputs[2])
    dead = ~(np.isfinite(film[..., :3]).all(-1) & np.isfinite(v))
    dead[h // 2, w // 2] = True
    assert bits_equal(got[dead][:, :3], film[dead][:, :3]) and bits_equal(gvar[dead], v[dead])   # dead pixels come out with their input bits
    assert np.all(np.isfinite(got[~dead])) and np.all(np.isfinite(gvar[~dead]))                  # ... and never spread


@pytest.mark.parametrize("w,h,seed", [(37, 23, 61), (70, 9, 62)])
def test_albedo_of_ones_and_of_none_equal_denoise_film(emu_al, pkg, w, h, seed):
    film, counts, stats, guides = td.synthetic_inputs(w, h, seed)
    want, wvar = emu_al.denoise_film(film, counts, stats, guides, variance=True)
    ones = np.ones((h, w, 4), F); ones[..., 3] = 0.0
    got, gvar = emu_al.denoise_film(film, counts, stats, guides, variance=True, albedo=ones)
    assert bits_equal(got, want) and bits_equal(gvar, wvar)
    fn = emu_al.lib.ptemu_denoise_film_albedo
    out, var = np.zeros((h, w, 4), F), np.zeros((h, w), F)
    d = pkg.api.DenoiseDesc(w, h, 0, 0.0, 0.0, 0, 0)
    assert fn(C.byref(d), film.ctypes.data_as(f32p), counts.ctypes.data_as(u32p), stats.ctypes.data_as(f64p), guides.ctypes.data_as(f32p), None,
              out.ctypes.data_as(f32p), var.ctypes.data_as(f32p)) == PT_OK
    assert bits_equal(out, want) and bits_equal(var, wvar)


def _albedo_refusals(fn, last_error, api, valid_status):
    W, H = 6, 5
    film, counts, stats, guides = td.synthetic_inputs(W, H, 3, dead=False)
    albedo = seeded_albedo(W, H, 4)
    out = np.zeros((H, W, 4), F)
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(api.DenoiseDesc), f32p, u32p, f64p, f32p, f32p, f32p, f32p]

    def status(alb, desc=None, counts_=counts):
        d = api.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0) if desc is None else desc
        return fn(C.byref(d), film.ctypes.data_as(f32p), counts_.ctypes.data_as(u32p), stats.ctypes.data_as(f64p), guides.ctypes.data_as(f32p),
                  None if alb is None else alb.ctypes.data_as(f32p), out.ctypes.data_as(f32p), None)

    assert status(albedo) == valid_status
    assert status(None) == valid_status
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        for where in ((0, 0, 0), (H - 1, W - 1, 2), (2, 3, 3)):
            a2 = albedo.copy(); a2[where] = bad
            assert status(a2) == PT_ERR_INVALID_ARGUMENT, (bad, where)
            assert b"albedo" in last_error()
    # a wrong size: the C entries see no array shapes, the film's size is the desc's — a desc of no pixels or of too many is refused ...
    assert status(albedo, api.DenoiseDesc(0, H, 0, 0.0, 0.0, 0, 0)) == PT_ERR_INVALID_ARGUMENT
    assert status(albedo, api.DenoiseDesc(1 << 16, 1 << 16, 0, 0.0, 0.0, 0, 0)) == PT_ERR_INVALID_ARGUMENT
    # ... and the rules of pt_denoise_film hold with an albedo
    c2 = counts.copy(); c2[0, 0] = 1
    assert status(albedo, counts_=c2) == PT_ERR_INVALID_ARGUMENT
    assert status(albedo, api.DenoiseDesc(W, H, 11, 0.0, 0.0, 0, 0)) == PT_ERR_INVALID_ARGUMENT


def test_emulation_refuses_a_bad_albedo(emu_al, pkg):
    err = emu_al.lib.ptemu_denoise_albedo_last_error
    err.restype = C.c_char_p
    _albedo_refusals(emu_al.lib.ptemu_denoise_film_albedo, err, pkg.api, PT_OK)
    # ... and the wrapper refuses an albedo of another film size before it calls
    film, counts, stats, guides = td.synthetic_inputs(6, 5, 3, dead=False)
    with pytest.raises(ValueError):
        emu_al.denoise_film(film, counts, stats, guides, albedo=np.ones((5, 7, 4), F))
    sc = emu_al.create_scene(pkg.scene.cornell_box())
    rd = pkg.api.render_desc(6, 5, 10, 3)
    g = np.zeros((5, 6, 4), F)
    fn = emu_al.lib.ptemu_render_guides_albedo
    assert fn(sc.handle, C.byref(rd), 2, g.ctypes.data_as(f32p), None) == PT_ERR_INVALID_ARGUMENT
    assert fn(sc.handle, C.byref(rd), 0, g.ctypes.data_as(f32p), g.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT
    assert fn(None, C.byref(rd), 2, g.ctypes.data_as(f32p), g.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT
    lam = np.zeros(16, F); xyz = np.zeros(48, F)
    bs = emu_al.lib.ptemu_albedo_basis
    assert bs(None, lam.ctypes.data_as(f32p), xyz.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT
    assert bs(C.byref(rd), None, xyz.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT
    assert bs(C.byref(pkg.api.render_desc(6, 5, 10, 3, wavelength=(700.0, 400.0))), lam.ctypes.data_as(f32p), xyz.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT


def test_engine_checks_the_albedo_before_it_looks_for_a_device(pkg):
    """pt_denoise_film_albedo takes no scene: its refusals need no GPU, and a valid call without a device is PT_ERR_NO_DEVICE."""
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_device_count.restype = C.c_uint32
    has_gpu = lib.pt_device_count() > 0
    _albedo_refusals(lib.pt_denoise_film_albedo, lib.pt_last_error, pkg.api, PT_OK if has_gpu else PT_ERR_NO_DEVICE)
    g = np.zeros((5, 6, 4), F)
    fn = lib.pt_render_guides_albedo
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(pkg.api.RenderDesc), C.c_uint32, f32p, f32p]
    assert fn(None, C.byref(pkg.api.render_desc(6, 5, 10, 3)), 2, g.ctypes.data_as(f32p), g.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT


def checker_mask(pkg, emu):
    """The pixels whose sample-0 camera ray hits the checker."""
    builder = pkg.scene.cornell_checker()
    sc = emu.create_scene(builder)
    rd = pkg.api.render_desc(48, 48, 20, td.BOUNCES, seed=1)
    n = 48 * 48
    o, d, _ = sc.camera_samples(rd, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32))
    h = sc.intersect(o, d)
    return ((h["valid"] != 0) & (h["material"] == builder.material("checker"))).reshape(48, 48)


def masked_rmse(a, b, mask):
    return float(np.sqrt(np.mean((a[mask][:, :3].astype(np.float64) - b[mask][:, :3].astype(np.float64)) ** 2)))


@pytest.mark.parametrize("spp", [20, 40])
def test_demodulation_protects_the_checker(emu_al, pkg, spp):
    """The issue's set-up: cornell_checker 48x48, seed 1, max_bounces 6, against 1000 spp of seed 77; RMSE over XYZ on the pixels whose sample-0 ray
    hits the checker (499 of them).  Measured in the emulation (noisy / denoise_film / demodulated): 20 spp 1.841e-3 / 1.685e-3 / 1.073e-3 (0.636 of the
    plain filter), whole-film ratio 0.590 -> 0.581, mean Y -1.84 % -> -1.19 %; 40 spp 1.247e-3 / 1.543e-3 / 0.953e-3 (0.618), whole film 0.727 -> 0.721 —
    at 40 spp the plain filter is worse than its input, the demodulated one is not.  The conditions are the orderings, no ratio."""
    film, counts, st, guides, albedo = checker_inputs(pkg, emu_al, spp)
    if "ref" not in _CHECKER:   # (one reference and one mask for both sample counts)
        _CHECKER["ref"] = emu_al.create_scene(pkg.scene.cornell_checker()).render(pkg.api.render_desc(48, 48, 1000, td.BOUNCES, seed=77))[0]
        _CHECKER["mask"] = checker_mask(pkg, emu_al)
    ref, mask = _CHECKER["ref"], _CHECKER["mask"]
    plain = emu_al.denoise_film(film, counts, st, guides)
    demod = emu_al.denoise_film(film, counts, st, guides, albedo=albedo)
    e_noisy, e_plain, e_demod = (masked_rmse(x, ref, mask) for x in (film, plain, demod))
    w_noisy, w_plain, w_demod = (td.film_rmse(x, ref) for x in (film, plain, demod))
    print("cornell_checker %d spp, %d checker pixels: rmse noisy %.4g, denoise_film %.4g, demodulated %.4g (%.3f of the plain filter); whole film %.4g / %.4g / %.4g "
          "(ratios %.3f, %.3f); mean Y %+.2f %% / %+.2f %%" % (spp, int(mask.sum()), e_noisy, e_plain, e_demod, e_demod / e_plain, w_noisy, w_plain, w_demod,
                                                                w_plain / w_noisy, w_demod / w_noisy, 100.0 * (plain[..., 1].mean() / film[..., 1].mean() - 1.0),
                                                                100.0 * (demod[..., 1].mean() / film[..., 1].mean() - 1.0)))
    assert e_demod < e_plain and e_demod < e_noisy
    assert w_demod < w_noisy


# ------------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("name", ALBEDO_SCENES + ("panorama_test",))
def test_gpu_albedo_equals_the_emulation(engine, emu_al, pkg, name):
    builder = builder_of(pkg, name)
    rd = pkg.api.render_desc(48, 48, 10, 4, seed=1)
    gsc, esc = engine.create_scene(builder), emu_al.create_scene(builder)
    guides, albedo = gsc.render_guides_albedo(rd, 4)
    eguides, ealbedo = esc.render_guides_albedo(rd, 4)
    assert bits_equal(guides, gsc.render_guides(rd, 4)) and bits_equal(guides, eguides)
    assert bits_equal(albedo, ealbedo), "%d values differ" % int((albedo.view(np.uint32) != ealbedo.view(np.uint32)).sum())


@pytest.mark.gpu
def test_gpu_albedo_equals_the_emulation_beyond_one_block(engine, emu_al, pkg):
    """70x45 = 3150 pixels: 13 blocks of 256 lanes, the last one partly filled; K = 1 and 3, other wavelength bounds."""
    builder = pkg.scene.cornell_checker(rgba=True)
    rd = pkg.api.render_desc(70, 45, 10, 4, seed=9, wavelength=(400.0, 700.0))
    gsc, esc = engine.create_scene(builder), emu_al.create_scene(builder)
    for K in (1, 3):
        got, want = gsc.render_guides_albedo(rd, K), esc.render_guides_albedo(rd, K)
        assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]), K


@pytest.mark.gpu
def test_gpu_basis_equals_the_emulation(engine, emu_al, pkg):
    for bounds in ((380.0, 750.0), (400.0, 700.0), (555.0, 555.0), (300.0, 900.0)):
        rd = pkg.api.render_desc(8, 8, 10, 3, wavelength=bounds)
        (lam, w), (elam, ew) = engine.albedo_basis(rd), emu_al.albedo_basis(rd)
        assert bits_equal(lam, elam) and bits_equal(w, ew), bounds


def check_albedo_against_emulation(engine, emu, inputs, **kw):
    film, counts, stats, guides, albedo = inputs
    got, gvar = engine.denoise_film(film, counts, stats, guides, variance=True, albedo=albedo, **kw)
    want, wvar = emu.denoise_film(film, counts, stats, guides, variance=True, albedo=albedo, **kw)
    assert bits_equal(got, want), "film: %d values differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(gvar, wvar), "variance: %d values differ" % int((gvar.view(np.uint32) != wvar.view(np.uint32)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("hero", [1, 4])
def test_gpu_filter_equals_the_emulation_on_the_rendered_checker(engine, emu_al, pkg, hero):
    sc = engine.create_scene(pkg.scene.cornell_checker())
    rd = pkg.api.render_desc(48, 48, 20, td.BOUNCES, seed=1, hero_wavelengths=hero)
    film, counts, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
    guides, albedo = sc.render_guides_albedo(rd, 4)
    check_albedo_against_emulation(engine, emu_al, (film, counts, st, guides, albedo))
    assert not bits_equal(engine.denoise_film(film, counts, st, guides, albedo=albedo), engine.denoise_film(film, counts, st, guides))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed,kw", [(37, 23, 61, {}), (70, 9, 62, td.OFF_DEFAULT), (257, 131, 63, {})])
def test_gpu_filter_equals_the_emulation_on_synthetic_inputs(engine, emu_al, w, h, seed, kw):
    """Films that straddle the 32x8 tiles, and one of many tiles with a ragged edge on both axes."""
    check_albedo_against_emulation(engine, emu_al, synthetic_with_albedo(w, h, seed), **kw)


@pytest.mark.gpu
def test_gpu_albedo_of_ones_and_of_none_equal_denoise_film(engine, pkg):
    w, h = 70, 9
    film, counts, stats, guides = td.synthetic_inputs(w, h, 62)
    want, wvar = engine.denoise_film(film, counts, stats, guides, variance=True)
    ones = np.ones((h, w, 4), F); ones[..., 3] = 0.0
    got, gvar = engine.denoise_film(film, counts, stats, guides, variance=True, albedo=ones)
    assert bits_equal(got, want) and bits_equal(gvar, wvar)
    out, var = np.zeros((h, w, 4), F), np.zeros((h, w), F)
    d = pkg.api.DenoiseDesc(w, h, 0, 0.0, 0.0, 0, 0)
    assert engine._denoise_film_albedo(C.byref(d), film.ctypes.data_as(f32p), counts.ctypes.data_as(u32p), stats.ctypes.data_as(f64p), guides.ctypes.data_as(f32p), None,
                                       out.ctypes.data_as(f32p), var.ctypes.data_as(f32p)) == PT_OK
    assert bits_equal(out, want) and bits_equal(var, wvar)


@pytest.mark.gpu
def test_gpu_render_denoised_with_albedo_equals_the_three_calls(engine, pkg):
    sc = engine.create_scene(pkg.scene.cornell_checker())
    rd = pkg.api.render_desc(64, 64, 20, 5, seed=2)
    film, den, counts, _ = sc.render_denoised(rd, albedo=True)
    f2, c2, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
    guides, albedo = sc.render_guides_albedo(rd, 4)
    want = engine.denoise_film(f2, c2, st, guides, albedo=albedo)
    assert bits_equal(film, f2) and np.array_equal(counts, c2) and bits_equal(den, want)
    plain = sc.render_denoised(rd)[1]
    assert bits_equal(plain, engine.denoise_film(f2, c2, st, guides)) and not bits_equal(plain, den)


@pytest.mark.gpu
def test_gpu_ptcli_demodulate_albedo(engine, pkg, tmp_path):
    """ptcli --denoise --demodulate-albedo writes the API's demodulated film into the <name>_denoised.* files; --denoise alone writes what it always
    wrote (the API's plain filter); the flag without --denoise is a usage error."""
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    text = open(os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c1.toml")).read()
    text = text.replace("min_samples = 16", "min_samples = 20").replace("width = 256", "width = 64").replace("height = 256", "height = 64")
    assert "min_samples = 20" in text and "width = 64" in text and "height = 64" in text
    cfg = tmp_path / "config.toml"
    cfg.write_text(text)
    runs = {}
    for tag, extra in (("denoise", ["--denoise"]), ("albedo", ["--denoise", "--demodulate-albedo"])):
        out = tmp_path / tag
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(out), "--write-film", "--seed", "5"] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = out
    names = ["beauty.exr", "beauty.npy", "beauty.png", "beauty_denoised.exr", "beauty_denoised.npy", "beauty_denoised.png"]
    assert sorted(os.listdir(runs["denoise"])) == names and sorted(os.listdir(runs["albedo"])) == names
    for f in ("beauty.exr", "beauty.npy", "beauty.png"):
        assert open(runs["denoise"] / f, "rb").read() == open(runs["albedo"] / f, "rb").read(), f
    sf = pkg.scene_file
    config = sf.Config(str(cfg))
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    rd = config.render_desc(0, seed=5)
    _, plain, _, _ = sc.render_denoised(rd)
    _, demod, _, _ = sc.render_denoised(rd, albedo=True)
    assert bits_equal(np.load(runs["denoise"] / "beauty_denoised.npy"), plain)
    assert bits_equal(np.load(runs["albedo"] / "beauty_denoised.npy"), demod)
    assert not bits_equal(plain, demod)
    assert open(runs["denoise"] / "beauty_denoised.png", "rb").read() != open(runs["albedo"] / "beauty_denoised.png", "rb").read()
    r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "refused"), "--demodulate-albedo"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=180)
    assert r.returncode != 0 and "--demodulate-albedo" in r.stderr and "--denoise" in r.stderr
    assert not (tmp_path / "refused").exists() or os.listdir(tmp_path / "refused") == []
