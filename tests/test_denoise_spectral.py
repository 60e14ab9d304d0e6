"""The adaptive spectral render and the joint filter of the film and its wavelength bins (pt_render_adaptive_spectral and pt_denoise_spectral of
include/pt_spectral.h).  The definition is exact, so every comparison is bit for bit unless a test says otherwise: the CPU tier
compares the host emulation (csrc/pt_denoise_spectral_rules.h compiled for the host, tests/host_emulation/ptemu_denoise_spectral.cpp) with a numpy
restatement written here and with the existing filter's emulation; the GPU tier compares the engine with the emulation, the adaptive bins with
pt_render_spectral at each pixel's own sample count, the composition with its parts, and the command line with the Python calls."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
from test_denoise import (OFF_DEFAULT, _inside, _tap, _two_class_inputs, bits_equal, np_kwargs, np_pt_exp, np_pt_min, np_variance, spread_rel,
                          synthetic_inputs)
from test_spectral import check_spectral_exr, scaled_c2_config
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_NO_DEVICE, PT_ERR_UNSUPPORTED, PT_OK

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
u32p, f64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_float)


@pytest.fixture(scope="session")
def emu_ds(pkg):
    """The host emulation with the adaptive driver, the film denoiser and the joint filter beside it: a library of its own."""
    L = emulation.load(pkg, "denoise_spectral")
    a = pkg.api
    L.lib.ptemu_denoise_spectral_last_error.restype = C.c_char_p
    L.lib.ptemu_spectral_finish.restype = C.c_int32
    L.lib.ptemu_spectral_finish.argtypes = [C.c_uint32, C.c_uint32, u32p, f32p]
    L.lib.ptemu_adaptive_spectral_check_args.restype = C.c_int32
    L.lib.ptemu_adaptive_spectral_check_args.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(a.SpectralDesc), C.c_uint32,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]
    return L


# ------------------------------------------------------------------------------------------------ numpy restatement of the definition
def np_denoise_spectral(film, counts, stats, guides, spectral, iterations=5, sl=4.0, sz=1.0, a=7):
    """pt_denoise_spectral in np.float32, in the rules header's order of operations: (film [H,W,4], variance [H,W], bins [B,H,W]).  The colour path is
    DESIGN.md section 13's (test_denoise.np_denoise restated, so that the weights are at hand); every bin plane is averaged with the same weights over
    the same taps, a tap that is not taken adds nothing, and a pixel with a non-finite bin is dead."""
    film = np.asarray(film, F); guides = np.asarray(guides, F)
    s = np.ascontiguousarray(np.moveaxis(np.asarray(spectral, F), 0, -1))   # [H,W,B]: _tap indexes the two leading axes
    h, w = counts.shape
    sl, sz = F(sl), F(sz)
    kern = [F(0.375), F(0.25), F(0.0625)]
    with np.errstate(all="ignore"):
        c = [film[..., k].copy() for k in range(3)]
        v = np_variance(counts, stats)
        dead = ~(np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & np.isfinite(v)) | ~np.isfinite(s).all(-1)
        nx, ny, nz, z = (guides[..., k] for k in range(4))
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        sky = ln == F(0.0)
        safe = np.where(sky, F(1.0), ln)
        nh = [np.where(sky, F(0.0), nx / safe), np.where(sky, F(0.0), ny / safe), np.where(sky, F(0.0), nz / safe)]
        gx, gy = np.zeros((h, w), F), np.zeros((h, w), F)
        if w >= 2:
            gx[:, 1:-1] = (z[:, 2:] - z[:, :-2]) * F(0.5); gx[:, 0] = z[:, 1] - z[:, 0]; gx[:, -1] = z[:, -1] - z[:, -2]
        if h >= 2:
            gy[1:-1] = (z[2:] - z[:-2]) * F(0.5); gy[0] = z[1] - z[0]; gy[-1] = z[-1] - z[-2]
        for it in range(iterations):
            st = 1 << it
            tsum, twsum = np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    g = F((2 - abs(dx)) * (2 - abs(dy)))
                    ok = _inside(h, w, dx, dy) & ~_tap(dead, dx, dy)
                    tsum = np.where(ok, tsum + g * _tap(v, dx, dy), tsum)
                    twsum = np.where(ok, twsum + g, twsum)
            vt = np.where(dead, F(0.0), tsum / twsum)
            sw, sv = np.zeros((h, w), F), np.zeros((h, w), F)
            sc = [np.zeros((h, w), F) for _ in range(3)]
            sb = np.zeros(s.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx * st, dy * st
                    inside = _inside(h, w, ox, oy)
                    if not inside.any():
                        continue
                    cq = [_tap(c[k], ox, oy) for k in range(3)]
                    vq = _tap(v, ox, oy)
                    if dx == 0 and dy == 0:
                        wgt = np.full((h, w), kern[0] * kern[0], F)
                        ok = inside
                    else:
                        skyq = _tap(sky, ox, oy)
                        ok = inside & ~_tap(dead, ox, oy) & (skyq == sky)
                        d = (nh[0] * _tap(nh[0], ox, oy) + nh[1] * _tap(nh[1], ox, oy)) + nh[2] * _tap(nh[2], ox, oy)
                        d = np.where(d > F(0.0), d, F(0.0))
                        for _ in range(a):
                            d = d * d
                        expected = np.abs(gx * F(ox) + gy * F(oy))
                        den = (sz * expected + F(1e-3) * np.abs(z)) + F(1e-30)
                        e = d * np_pt_exp(-np_pt_min(np.abs(z - _tap(z, ox, oy)) / den, F(80.0)))
                        e = np.where(sky, F(1.0), e)
                        lum = np_pt_exp(-np_pt_min(np.abs(c[1] - cq[1]) / (sl * np.sqrt(vt + _tap(vt, ox, oy)) + F(1e-20)), F(80.0)))
                        wgt = ((kern[abs(dx)] * kern[abs(dy)]) * e) * lum
                    sw = np.where(ok, sw + wgt, sw)
                    for k in range(3):
                        sc[k] = np.where(ok, sc[k] + wgt * cq[k], sc[k])
                    sv = np.where(ok, sv + (wgt * wgt) * vq, sv)
                    sb = np.where(ok[..., None], sb + wgt[..., None] * _tap(s, ox, oy), sb)
            c = [np.where(dead, c[k], sc[k] / sw) for k in range(3)]
            v = np.where(dead, v, sv / (sw * sw))
            s = np.where(dead[..., None], s, sb / sw[..., None])
        out = np.zeros((h, w, 4), F)
        for k in range(3):
            out[..., k] = c[k]
        return out, v.astype(F), np.ascontiguousarray(np.moveaxis(s, -1, 0)).astype(F)


# ------------------------------------------------------------------------------------------------ inputs
SIZES = [(64, 40, 11), (37, 53, 12), (5, 3, 13), (1, 9, 14), (9, 1, 15)]   # (width, height, seed)
BINS = (1, 3, 7, 9, 64)


def params_for(w, h):
    """Default and off-default parameters; on the 5x3 film also ten passes, so that every far tap is outside."""
    return [{}, OFF_DEFAULT] + ([dict(iterations=10, normal_power_log2=10, sigma_luminance=0.25, sigma_depth=8.0)] if (w, h) == (5, 3) else [])


def synthetic_spectral(inputs, B, seed, bin_dead=True):
    """Bins for test_denoise.synthetic_inputs (which hold sky pixels and pixels dead through the film or the statistics): per pixel a random split of the
    film's Y over B bins plus noise, NaN where the film is not finite (so that the planes 0..2 may stand in for X, Y, Z), and — with `bin_dead` — one pixel,
    live by its film, dead only through one infinite bin.  Returns (spectral [B,H,W], (y, x) of that pixel or None)."""
    film = inputs[0]
    h, w = film.shape[:2]
    rng = np.random.default_rng(seed * 131 + B)
    split = rng.dirichlet(np.ones(B), (h, w)).astype(F)                     # [H,W,B]
    noise = F(1.0) + F(0.3) * rng.standard_normal((h, w, B)).astype(F)
    with np.errstate(all="ignore"):
        s = np.moveaxis(film[..., 1:2] * split * noise, -1, 0)
    s = np.ascontiguousarray(s, F)
    where = None
    if bin_dead:
        live = np.isfinite(film[..., :3]).all(-1) & np.isfinite(np_variance(inputs[1], inputs[2]))
        ys, xs = np.nonzero(live)
        k = np.argmin(np.abs(ys - h // 2) + np.abs(xs - w // 2))             # the live pixel nearest the centre
        where = (int(ys[k]), int(xs[k]))
        s[B // 2, where[0], where[1]] = np.inf
    return s, where


def emu_call(lib, inputs, spectral, **kw):
    """(film, variance, bins)"""
    out, out_spectral, var = lib.denoise_spectral(*inputs, spectral, variance=True, **kw)
    return out, var, out_spectral


# ------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("w,h,seed", SIZES)
def test_filter_equals_the_numpy_restatement_on_synthetic_inputs(emu_ds, w, h, seed, B):
    """Film, variance and every bin plane against numpy; the dead pixels — through the film, the statistics, or one bin alone — come out as they went in,
    and nothing they hold spreads."""
    inputs = synthetic_inputs(w, h, seed)
    spectral, where = synthetic_spectral(inputs, B, seed)
    film = inputs[0]
    dead = ~np.isfinite(film[..., :3]).all(-1) | ~np.isfinite(np_variance(inputs[1], inputs[2])) | ~np.isfinite(spectral).all(0)
    assert dead[where] and np.isfinite(film[where][:3]).all() and (~dead).any()
    for kw in params_for(w, h):
        got, gvar, gsp = emu_call(emu_ds, inputs, spectral, **kw)
        want, wvar, wsp = np_denoise_spectral(*inputs, spectral, **np_kwargs(kw))
        assert bits_equal(got, want), (kw, "film: %d values differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert bits_equal(gvar, wvar), kw
        assert bits_equal(gsp, wsp), (kw, "bins: %d values differ" % int((gsp.view(np.uint32) != wsp.view(np.uint32)).sum()))
        assert bits_equal(got[dead][:, :3], film[dead][:, :3]) and bits_equal(gsp[:, dead], spectral[:, dead])
        assert np.all(np.isfinite(gsp[:, ~dead])) and np.all(np.isfinite(got[~dead]))
        assert np.all(got[..., 3] == 0.0)


IDENTITY = (37, 53, 12)


def test_bins_that_hold_the_film_come_out_as_the_film(emu_ds):
    """Identities 1 and 2: with bins 0, 1, 2 set to the film's X, Y, Z planes the output bins are ptemu_denoise_film's X, Y, Z planes, and out_film and
    out_variance are ptemu_denoise_film's (a pixel whose film is not finite has non-finite bins here: dead either way)."""
    w, h, seed = IDENTITY
    inputs = synthetic_inputs(w, h, seed)
    spectral = np.ascontiguousarray(np.moveaxis(inputs[0][..., :3], -1, 0))
    for kw in ({}, OFF_DEFAULT):
        got, gvar, gsp = emu_call(emu_ds, inputs, spectral, **kw)
        want, wvar = emu_ds.denoise_film(*inputs, variance=True, **kw)
        assert bits_equal(got, want) and bits_equal(gvar, wvar)
        for k in range(3):
            assert bits_equal(gsp[k], want[..., k]), k


def test_each_plane_of_a_wide_call_is_the_one_bin_call(emu_ds):
    """Identity 3: plane b of a B = 64 call (eight chunks of 8) and of a B = 7 call (the remainder's chunks of 4, 2 and 1) equals the B = 1 call on that
    plane alone.  The bins are finite everywhere, so that both calls have the same dead pixels."""
    w, h, seed = IDENTITY
    inputs = synthetic_inputs(w, h, seed)
    for B in (64, 7):
        spectral, _ = synthetic_spectral(inputs, B, seed, bin_dead=False)
        spectral = np.where(np.isfinite(spectral), spectral, F(0.25))
        _, _, wide = emu_call(emu_ds, inputs, spectral)
        for b in sorted({0, 3, 4, 5, 6, 7, 8, 31, 56, 62, 63} & set(range(B))):
            _, _, one = emu_call(emu_ds, inputs, spectral[b:b + 1])
            assert bits_equal(wide[b], one[0]), (B, b)


def test_scaled_bins_give_scaled_outputs_and_a_constant_plane_stays_constant(emu_ds):
    """Identity 4: bins times 2.0f give outputs times 2.0f (a power of two commutes with every rounding here: no value is near the subnormals).
    Identity 5: a plane of zeros stays +0 exactly, and a constant plane returns the constant within I x 64 x 2^-24 relative — per pass 25 products and 24
    additions in the numerator, 24 additions in the weight sum, one division: at most 50 roundings of 2^-24 each (test_denoise's bound for the film)."""
    w, h, seed = IDENTITY
    inputs = synthetic_inputs(w, h, seed)
    spectral, _ = synthetic_spectral(inputs, 9, seed)
    _, _, a = emu_call(emu_ds, inputs, spectral)
    _, _, b = emu_call(emu_ds, inputs, spectral * F(2.0))
    assert bits_equal(a * F(2.0), b)
    live = np.isfinite(inputs[0][..., :3]).all(-1) & np.isfinite(np_variance(inputs[1], inputs[2]))
    for iterations in (1, 5, 10):
        const = np.zeros((3, h, w), F)
        const[1], const[2] = F(0.7312), F(1903.1)
        _, _, out = emu_call(emu_ds, inputs, const, iterations=iterations)
        assert np.all(out[0].view(np.uint32) == 0)
        for k in (1, 2):
            rel = np.abs(out[k][live].astype(np.float64) - float(const[k, 0, 0])) / float(const[k, 0, 0])
            print("constant plane %d, %d passes: largest relative deviation %.3g (bound %.3g)" % (k, iterations, rel.max(), iterations * 64 * 2.0 ** -24))
            assert rel.max() <= iterations * 64 * 2.0 ** -24


@pytest.mark.parametrize("right_guides", [(0.0, 1.0, 0.0, 3.0), (0.0, 0.0, 0.0, 0.0)], ids=["orthogonal_normals", "sky"])
def test_no_bin_crosses_an_edge(emu_ds, right_guides):
    """Identity 6, test_nothing_crosses_an_edge's construction: two half-planes with orthogonal normals, and surface against sky.  Changing the right half's
    bins leaves the left half's output bins bit-identical — a tap across the edge has weight 0 or is skipped — for one, five and ten passes: the weights
    come from the film and the guides, which do not change."""
    rng = np.random.default_rng(8)
    film, counts, stats, guides, left = _two_class_inputs(48, 40, 21, right_guides, False)
    inputs = (film, counts, stats, guides)
    spectral, _ = synthetic_spectral(inputs, 9, 21, bin_dead=False)
    other = spectral.copy()
    other[:, ~left] = (spectral[:, ~left] * rng.uniform(0.0, 30.0, spectral[:, ~left].shape)).astype(F) + F(0.5)
    for iterations in (1, 5, 10):
        fa, _, a = emu_call(emu_ds, inputs, spectral, iterations=iterations)
        fb, _, b = emu_call(emu_ds, inputs, other, iterations=iterations)
        assert bits_equal(fa, fb)
        assert bits_equal(a[:, left], b[:, left]), iterations
        assert not bits_equal(a[:, ~left], b[:, ~left])


def test_finish_rule_divides_each_pixel_by_its_own_count(emu_ds):
    """spectral_finish_value: S / (float)n per bin, with counts of 10, 20 and 4090; a count of 0 leaves the value."""
    rng = np.random.default_rng(3)
    counts = np.array([10, 20, 4090, 10, 4090, 0, 20], np.uint32)
    sums = (rng.exponential(50.0, (5, counts.size))).astype(F)
    sums[0, 1], sums[4, 2], sums[2, 5] = 0.0, np.inf, 7.5
    got = sums.copy()
    assert emu_ds.lib.ptemu_spectral_finish(counts.size, 5, counts.ctypes.data_as(u32p), got.ctypes.data_as(f32p)) == PT_OK
    n = np.where(counts == 0, 1, counts).astype(F)
    want = np.where(counts == 0, sums, sums / n[None, :])
    assert bits_equal(got, want)
    assert got[2, 5] == F(7.5) and got[0, 0] == sums[0, 0] / F(10.0) and got[1, 2] == sums[1, 2] / F(4090.0)


def _denoise_spectral_refusals(fn, last_error, a, valid_status):
    """Every rule of pt_denoise_spectral's arguments against one library; `valid_status`: what a valid call returns."""
    W, H, B = 6, 5, 3
    film, counts, stats, guides = synthetic_inputs(W, H, 3, dead=False)
    spectral = np.ones((B, H, W), F)
    out, osp, var = np.zeros((H, W, 4), F), np.zeros((B, H, W), F), np.zeros((H, W), F)
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(a.DenoiseDesc), C.c_uint32, f32p, u32p, f64p, f32p, f32p, f32p, f32p, f32p]
    P = dict(film=film.ctypes.data_as(f32p), counts=counts.ctypes.data_as(u32p), stats=stats.ctypes.data_as(f64p), guides=guides.ctypes.data_as(f32p),
             spectral=spectral.ctypes.data_as(f32p), out=out.ctypes.data_as(f32p), osp=osp.ctypes.data_as(f32p), var=var.ctypes.data_as(f32p))
    msgs = {}

    def status(key, bins=B, desc=None, null_desc=False, **over):
        p = dict(P); p.update(over)
        d = a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0) if desc is None else desc
        st = fn(None if null_desc else C.byref(d), bins, p["film"], p["counts"], p["stats"], p["guides"], p["spectral"], p["out"], p["osp"], p["var"])
        if st not in (PT_OK, PT_ERR_NO_DEVICE):
            msgs[key] = last_error().decode()
        return st

    assert status("ok") == valid_status
    assert status("ok", var=None) == valid_status                          # (out_variance may be NULL)
    assert status("ok", osp=P["spectral"]) == valid_status                 # (out_spectral may be spectral)
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
    assert "ok" not in msgs and all(msgs.values()) and len(set(msgs.values())) == len(msgs), msgs
    assert "bins" in msgs["zero"] and "64" in msgs["many"] and "spectral" in msgs["spectral"] and "out_spectral" in msgs["out_spectral"]
    assert "sample count below 2" in msgs["count"] and "guide" in msgs["guide"] and "iterations" in msgs["iterations"]


def test_emulation_refuses_each_bad_filter_argument(emu_ds, pkg):
    _denoise_spectral_refusals(emu_ds.lib.ptemu_denoise_spectral, emu_ds.lib.ptemu_denoise_spectral_last_error, pkg.api, PT_OK)


def test_engine_checks_the_filter_arguments_before_it_looks_for_a_device(pkg):
    """pt_denoise_spectral takes no scene: its refusals need no GPU, and a valid call without a device is PT_ERR_NO_DEVICE (there is no CPU fallback)."""
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_device_count.restype = C.c_uint32
    has_gpu = lib.pt_device_count() > 0
    _denoise_spectral_refusals(lib.pt_denoise_spectral, lib.pt_last_error, pkg.api, PT_OK if has_gpu else PT_ERR_NO_DEVICE)
    if not has_gpu:
        film, counts, stats, guides = synthetic_inputs(6, 5, 3, dead=False)
        with pytest.raises(pkg.api.PtError, match="no CPU fallback"):
            pkg.load().denoise_spectral(film, counts, stats, guides, np.ones((2, 5, 6), F))


def test_an_albedo_is_refused_as_unsupported(pkg):
    """There is no albedo form of the joint filter: the Python layer refuses one with PT_ERR_UNSUPPORTED before anything runs."""
    film, counts, stats, guides = synthetic_inputs(6, 5, 3, dead=False)
    with pytest.raises(pkg.api.PtError, match="per-bin albedo") as e:
        pkg.load().denoise_spectral(film, counts, stats, guides, np.ones((2, 5, 6), F), albedo=np.ones((5, 6, 4), F))
    assert e.value.status == PT_ERR_UNSUPPORTED


def test_adaptive_spectral_arguments_are_refused_each_with_its_own_message(emu_ds, pkg):
    """pth::check_adaptive_spectral_args, the checker pt_render_adaptive_spectral runs before it touches a device: pt_render_adaptive's conditions and
    check_spectral_args's.  The engine's own entry refuses a null scene on any machine."""
    a = pkg.api
    buf = np.zeros(4, F)
    ptr = buf.ctypes.data
    msgs = {}
    check = emu_ds.lib.ptemu_adaptive_spectral_check_args

    def status(key, scene=ptr, rd=None, ad=None, sd=None, cameras=1, film=ptr, counts=ptr, spectral=ptr):
        rd = a.render_desc(8, 8, 10, 3) if rd is None else rd
        ad = a.AdaptiveDesc(40, 10, 0.05, 0.0) if ad is None else ad
        sd = a.SpectralDesc(5) if sd is None else sd
        st = check(scene, None if rd == "null" else C.byref(rd), None if ad == "null" else C.byref(ad), None if sd == "null" else C.byref(sd), cameras, film, counts, spectral)
        if st != PT_OK:
            msgs[key] = emu_ds.lib.ptemu_denoise_spectral_last_error().decode()
        return st

    assert status("ok") == PT_OK
    assert status("ok", ad=a.AdaptiveDesc(10, 0, 0.0, 0.0), sd=a.SpectralDesc(64)) == PT_OK
    assert status("ok", rd=a.render_desc(8, 8, 10, 3, hero_wavelengths=4)) == PT_OK
    assert status("scene", scene=None) == PT_ERR_INVALID_ARGUMENT
    assert status("rd", rd="null") == PT_ERR_INVALID_ARGUMENT
    assert status("ad", ad="null") == PT_ERR_INVALID_ARGUMENT
    assert status("sd", sd="null") == PT_ERR_INVALID_ARGUMENT
    assert status("zero", sd=a.SpectralDesc(0)) == PT_ERR_INVALID_ARGUMENT
    assert status("many", sd=a.SpectralDesc(65)) == PT_ERR_INVALID_ARGUMENT
    sd = a.SpectralDesc(5); sd.reserved[2] = 1
    assert status("reserved", sd=sd) == PT_ERR_INVALID_ARGUMENT
    assert status("film", film=None) == PT_ERR_INVALID_ARGUMENT
    assert status("spectral", spectral=None) == PT_ERR_INVALID_ARGUMENT
    assert status("counts", counts=None) == PT_ERR_INVALID_ARGUMENT
    assert status("phase", rd=a.render_desc(8, 8, 10, 3, phase_samples=5)) == PT_ERR_UNSUPPORTED
    assert status("shard", rd=a.render_desc(8, 8, 10, 3, shard=(0, 2))) == PT_ERR_UNSUPPORTED
    assert status("range", rd=a.render_desc(8, 8, 10, 3, first_sample=0, sample_count=10)) == PT_ERR_INVALID_ARGUMENT
    assert status("tens", rd=a.render_desc(8, 8, 16, 3)) == PT_ERR_INVALID_ARGUMENT
    assert status("tens", ad=a.AdaptiveDesc(40, 5, 0.05, 0.0)) == PT_ERR_INVALID_ARGUMENT
    assert status("max", ad=a.AdaptiveDesc(0, 10, 0.05, 0.0)) == PT_ERR_INVALID_ARGUMENT
    assert status("error", ad=a.AdaptiveDesc(40, 10, -1.0, 0.0)) == PT_ERR_INVALID_ARGUMENT
    assert status("camera", cameras=0) == PT_ERR_INVALID_ARGUMENT
    assert "ok" not in msgs and all(msgs.values()) and len(set(msgs.values())) == len(msgs), msgs
    assert "bins" in msgs["zero"] and "64" in msgs["many"] and "reserved" in msgs["reserved"] and "sample_counts" in msgs["counts"] and "multiples of 10" in msgs["tens"]
    # the engine: before a device is looked for (and before the scene is read)
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    fn = lib.pt_render_adaptive_spectral
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(a.SpectralDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rd, ad, sd = a.render_desc(8, 8, 10, 3), a.AdaptiveDesc(40, 10, 0.05, 0.0), a.SpectralDesc(5)
    assert fn(None, C.byref(rd), C.byref(ad), C.byref(sd), ptr, ptr, None, ptr, None) == PT_ERR_INVALID_ARGUMENT
    assert lib.pt_last_error().decode() == msgs["scene"]


def test_library_exports_the_entries_and_the_header_stands_alone(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ("pt_render_adaptive_spectral", "pt_denoise_spectral"):
        assert hasattr(lib, name), name
    assert not any("spectral" in f for f in pkg.api.API_FUNCTIONS)   # (pt_api.h's list: the boundary the oracle shares)
    text = open(os.path.join(ROOT, "include", "pt_spectral.h")).read()
    for name in ("pt_render_adaptive_spectral", "pt_denoise_spectral"):
        assert re.search(r"pt_status %s\(" % name, text), name
    # pt_spectral.h brings the descs of the two entries with it, and the Python structs have their sizes
    src = '#include <stdio.h>\n#include "pt_spectral.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(pt_adaptive_desc), sizeof(pt_denoise_desc), sizeof(pt_spectral_desc)); return 0; }'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    a = pkg.api
    assert out == [C.sizeof(a.AdaptiveDesc), C.sizeof(a.DenoiseDesc), C.sizeof(a.SpectralDesc)]
    e = pkg.load()
    assert e._render_adaptive_spectral is not None and e._denoise_spectral is not None


# ------------------------------------------------------------------------------------------------ GPU tier
GW, GH, BOUNCES, GB = 32, 32, 4, 8
BOUNDS = (380.0, 750.0)
ADAPTIVE_SCENES = {"cornell_hero": ("cornell_box", dict(hero_wavelengths=4)), "hdri": ("hdri_small", dict())}   # test_spectral.CASES' two smallest, one with four wavelengths


def adaptive_rd(pkg, kw):
    return pkg.api.render_desc(GW, GH, 10, BOUNCES, seed=7, wavelength=BOUNDS, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ADAPTIVE_SCENES))
def test_gpu_adaptive_bins_equal_the_fixed_render_at_each_pixels_count(engine, pkg, name):
    """spp 10, max_samples 40, step 10.  rel_error is test_denoise.spread_rel's: the 0.8-quantile of the pixels' own relative errors after round 0, so that
    a fifth of the pixels (and, through the 3x3 rule, their neighbours) go on while the rest may stop — chosen from the render itself, not from a scene's
    brightness, so that at least two counts occur.  film, counts and stats are render_adaptive's; the bins of the pixels that stopped at n are
    render_spectral(spp = n)'s; with rel_error 0 everything is render_spectral(spp = 40)'s; a small batch_slots, which continues pixels across passes,
    changes no bit."""
    make, kw = ADAPTIVE_SCENES[name]
    builder = getattr(pkg.scene, make)()
    rd = adaptive_rd(pkg, kw)
    rel = spread_rel(engine, builder, rd, 0.8)
    sc = engine.create_scene(builder)
    film, counts, st, spectral, prof = sc.render_adaptive_spectral(rd, GB, 40, rel, step=10, stats=True)
    f2, c2, s2, p2 = sc.render_adaptive(rd, 40, rel, step=10, stats=True)
    print("%s: rel_error %.4g, counts %s" % (name, rel, dict(zip(*[x.tolist() for x in np.unique(counts, return_counts=True)]))))
    assert len(np.unique(counts)) >= 2, np.unique(counts)
    assert film.tobytes() == f2.tobytes() and np.array_equal(counts, c2) and st.tobytes() == s2.tobytes()
    assert (prof.camera_rays, prof.bounce_rays, prof.shadow_rays, prof.kernel_launches[5]) == (p2.camera_rays, p2.bounce_rays, p2.shadow_rays, p2.kernel_launches[5])
    assert np.any(spectral != 0)
    for n in np.unique(counts):
        fixed_film, fixed, _ = sc.render_spectral(pkg.api.render_desc(GW, GH, int(n), BOUNCES, seed=7, wavelength=BOUNDS, **kw), GB)
        at = counts == n
        assert bits_equal(spectral[:, at], fixed[:, at]), int(n)
        assert bits_equal(film[at], fixed_film[at]), int(n)
    film0, counts0, spectral0, _ = sc.render_adaptive_spectral(rd, GB, 40, 0.0, step=10)
    fixed_film, fixed, _ = sc.render_spectral(pkg.api.render_desc(GW, GH, 40, BOUNCES, seed=7, wavelength=BOUNDS, **kw), GB)
    assert np.all(counts0 == 40) and bits_equal(spectral0, fixed) and film0.tobytes() == fixed_film.tobytes()
    t = engine.tuning_default()
    t.batch_slots = 1024
    small = engine.create_scene(builder, tuning=t).render_adaptive_spectral(rd, GB, 40, rel, step=10, stats=True)
    assert small[4].kernel_launches[0] > prof.kernel_launches[0]                  # (more generate launches: more passes)
    assert small[0].tobytes() == film.tobytes() and np.array_equal(small[1], counts) and bits_equal(small[3], spectral)


def check_against_emulation(engine, emu, inputs, spectral, **kw):
    got, gsp, gvar = engine.denoise_spectral(*inputs, spectral, variance=True, **kw)
    want, wsp, wvar = emu.denoise_spectral(*inputs, spectral, variance=True, **kw)
    assert bits_equal(got, want), "film: %d values differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(gvar, wvar), "variance: %d values differ" % int((gvar.view(np.uint32) != wvar.view(np.uint32)).sum())
    assert bits_equal(gsp, wsp), "bins: %d values differ" % int((gsp.view(np.uint32) != wsp.view(np.uint32)).sum())
    return got, gsp


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", SIZES)
def test_gpu_filter_equals_the_emulation_on_synthetic_inputs(engine, emu_ds, w, h, seed):
    """The CPU tier's inputs, sizes, bin counts and parameters through the engine."""
    inputs = synthetic_inputs(w, h, seed)
    for B in BINS:
        spectral, _ = synthetic_spectral(inputs, B, seed)
        for kw in params_for(w, h):
            check_against_emulation(engine, emu_ds, inputs, spectral, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ADAPTIVE_SCENES))
def test_gpu_filter_equals_the_emulation_on_a_rendered_input(engine, emu_ds, pkg, name):
    """render_adaptive_spectral plus render_guides of one scene through both filters; out_film is denoise_film's."""
    make, kw = ADAPTIVE_SCENES[name]
    sc = engine.create_scene(getattr(pkg.scene, make)())
    rd = pkg.api.render_desc(48, 32, 20, BOUNCES, seed=3, wavelength=BOUNDS, **kw)
    film, counts, st, spectral, _ = sc.render_adaptive_spectral(rd, GB, 40, 0.05, step=10, stats=True)
    guides = sc.render_guides(rd, 4)
    got, gsp = check_against_emulation(engine, emu_ds, (film, counts, st, guides), spectral)
    assert bits_equal(got, engine.denoise_film(film, counts, st, guides))
    assert not bits_equal(gsp, spectral)


@pytest.mark.gpu
def test_gpu_render_denoised_spectral_equals_the_calls_made_by_hand(engine, pkg):
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_box())
    rd = a.render_desc(GW, GH, 20, BOUNCES, seed=2, wavelength=BOUNDS)
    film, den, spectral, den_spectral, counts, prof = sc.render_denoised_spectral(rd, GB, max_samples=40, rel_error=0.05, guide_samples=2, iterations=3, sigma_luminance=2.0)
    f2, c2, st, s2, _ = sc.render_adaptive_spectral(rd, GB, 40, 0.05, stats=True)
    d2, ds2 = engine.denoise_spectral(f2, c2, st, sc.render_guides(rd, 2), s2, iterations=3, sigma_luminance=2.0)
    assert bits_equal(film, f2) and np.array_equal(counts, c2) and bits_equal(spectral, s2) and bits_equal(den, d2) and bits_equal(den_spectral, ds2)
    assert prof.camera_rays == int(counts.sum()) and not bits_equal(den_spectral, spectral)
    with pytest.raises(a.PtError, match="per-bin albedo"):
        sc.render_denoised_spectral(rd, GB, albedo=True)
    slab = engine.create_scene(pkg.scene.cornell_checker_slab())
    film, den, spectral, den_spectral, counts, _ = slab.render_denoised_spectral(rd, GB, specular_chain=8)
    f2, c2, st, s2, _ = slab.render_adaptive_spectral(rd, GB, 20, 0.0, stats=True)
    chain_guides, _ = slab.render_guides_chain(rd, 4, 8, albedo=False)
    d2, ds2 = engine.denoise_spectral(f2, c2, st, chain_guides, s2)
    assert bits_equal(film, f2) and bits_equal(spectral, s2) and bits_equal(den, d2) and bits_equal(den_spectral, ds2)
    assert not bits_equal(chain_guides, slab.render_guides(rd, 4))                # (the chain does change the guides here)


def bins_sse(a, b):
    return float(np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.gpu
def test_gpu_denoised_bins_are_closer_to_a_converged_spectral_render(engine, pkg):
    """Cornell box, 32x32, 20 spp, 8 bins, defaults, against render_spectral at 4000 spp of another seed: the denoised bins' summed squared error is strictly
    below the noisy bins'.  No threshold is set; both numbers are printed (measured on an MI355X: 6.01 and 2.26).  (tools/denoise_quality.py --size 32 --spp 20 --ref-spp 4000 --spectral-bins 8 writes
    them, per scene, into profiles/denoise_quality.json under gpu_32_spectral8.)"""
    sc = engine.create_scene(pkg.scene.cornell_box())
    rd = pkg.api.render_desc(GW, GH, 20, 6, seed=1, wavelength=BOUNDS)
    _, _, spectral, den_spectral, _, _ = sc.render_denoised_spectral(rd, GB)
    _, ref, _ = sc.render_spectral(pkg.api.render_desc(GW, GH, 4000, 6, seed=77, wavelength=BOUNDS), GB)
    e0, e1 = bins_sse(spectral, ref), bins_sse(den_spectral, ref)
    print("bins: summed squared error noisy %.6g, denoised %.6g, ratio %.3f" % (e0, e1, e1 / e0))
    assert e1 < e0


@pytest.mark.gpu
def test_gpu_ptcli_denoise_spectral_bins(engine, pkg, tmp_path):
    """ptcli --denoise --denoise-spectral-bins 8 on test_spectral's scaled C2 config: the usual and the _denoised files are byte for byte those of --denoise
    alone; <name>_spectral.exr and <name>_denoised_spectral.exr hold render_denoised_spectral's bins times the factor beside the R, G, B of the film and of
    the denoised film; the refused combinations exit non-zero with their messages; the help text names the flag."""
    sf = pkg.scene_file
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    plain, spec = run("plain", "--denoise"), run("spec", "--denoise", "--denoise-spectral-bins", "8")
    assert plain.returncode == 0 and spec.returncode == 0, plain.stdout + plain.stderr + spec.stdout + spec.stderr
    assert "beauty_spectral.exr (8 bins)" in spec.stdout and "beauty_denoised_spectral.exr (8 bins)" in spec.stdout
    usual = ["beauty.exr", "beauty.png", "beauty_denoised.exr", "beauty_denoised.png"]
    assert sorted(os.listdir(tmp_path / "plain")) == usual
    assert sorted(os.listdir(tmp_path / "spec")) == sorted(usual + ["beauty_spectral.exr", "beauty_denoised_spectral.exr"])
    for f in usual:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "spec" / f).read_bytes(), f
    config = sf.Config(str(cfg))
    rd, od = config.render_desc(0, seed=1), config.output_desc(0)
    assert (rd.width, rd.height, rd.spp) == (32, 32, 20) and od.factor == 2.0
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    film, den, spectral, den_spectral, _, _ = sc.render_denoised_spectral(rd, 8)
    centres = engine.spectral_bin_centres(rd, 8)
    for name, f, s in (("beauty_spectral.exr", film, spectral), ("beauty_denoised_spectral.exr", den, den_spectral)):
        _, linear = engine.output_film(f, od.tonemap, od.luminance_only, od.exposure, od.key_value, od.white_point, od.colorspace, od.factor)
        check_spectral_exr(str(tmp_path / "spec" / name), centres, s * F(od.factor), linear)
    assert not bits_equal(den_spectral, spectral)
    for extra, message in ((["--denoise-spectral-bins", "8"], "--denoise-spectral-bins needs --denoise"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--spectral-bins", "8"], "--denoise-spectral-bins cannot be combined with --spectral-bins"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--demodulate-albedo"], "--denoise-spectral-bins cannot be combined with --demodulate-albedo"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--devices", "3"], "--denoise-spectral-bins renders on device 0"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--devices", "0"], "--denoise-spectral-bins renders on device 0"),
                           (["--denoise", "--denoise-spectral-bins", "0"], "--denoise-spectral-bins needs a count in 1..64"),
                           (["--denoise", "--denoise-spectral-bins", "65"], "--denoise-spectral-bins needs a count in 1..64")):
        r = run("refused", *extra)
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "refused" / "beauty.exr").exists()
    assert run("one", "--denoise", "--denoise-spectral-bins", "8", "--devices", "1").returncode == 0
    assert (tmp_path / "one" / "beauty_spectral.exr").read_bytes() == (tmp_path / "spec" / "beauty_spectral.exr").read_bytes()
    assert "--denoise-spectral-bins" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
