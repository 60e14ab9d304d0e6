"""The film denoiser (include/pt_denoise.h): guides from the two probes, the variance of the mean from the adaptive render's
statistics, and the edge-avoiding a-trous filter.  The definition is exact (f32 data flow in a fixed order, pt_exp of include/pt_numerics.h), so every
check is bit for bit: the CPU tier compares the host emulation (the rules header compiled for the host) with a numpy restatement written operation by
operation and with the oracle's probes; the GPU tier compares the engine with the emulation."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_NO_DEVICE, PT_OK, bits_equal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
u32p, f64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_float)


@pytest.fixture(scope="session")
def emu_dn(pkg):
    """The host emulation with the adaptive driver (the statistics come from ptemu_render_adaptive) and the denoiser beside it: a library of its own."""
    return emulation.load(pkg, "denoise")


# ------------------------------------------------------------------------------------------------ numpy restatement of the definition
def np_pt_min(a, b):
    """pt_min: the non-NaN operand if one is NaN."""
    return np.where((a <= b) | (b != b), a, b)


def np_pt_floor(x):
    t = x.astype(np.int32).astype(F)
    return np.where(t > x, t - F(1.0), t)


def np_pt_exp(x0):
    """pt_exp of include/pt_numerics.h: pure f32 arithmetic, restated step by step."""
    x0 = np.asarray(x0, F)
    is_nan, over, under = x0 != x0, x0 > F(88.72283905206835), x0 < F(-103.9)
    x = np.where(is_nan | over | under, F(0.0), x0)
    fn = np_pt_floor(F(1.44269504088896341) * x + F(0.5))
    n = fn.astype(np.int32)
    x = x - fn * F(0.693359375)
    x = x - fn * F(-2.12194440e-4)
    z = x * x
    p = (((((F(1.9875691500e-4) * x + F(1.3981999507e-3)) * x + F(8.3334519073e-3)) * x + F(4.1665795894e-2)) * x + F(1.6666665459e-1)) * x + F(5.0000001201e-1)) * z + x + F(1.0)
    hi = n > 127
    p = np.where(hi, p * F(2.0), p); n = np.where(hi, n - 1, n)
    sub = n < -126
    p = np.where(sub, p * F(5.42101086242752217e-20), p); n = np.where(sub, n + 64, n)
    gone = n < -126
    scale = ((np.where(gone, 0, n) + 127).astype(np.uint32) << np.uint32(23)).view(F)
    r = p * scale
    r = np.where(gone | under, F(0.0), r)
    r = np.where(over, F(np.inf), r)
    return np.where(is_nan, x0, r).astype(F)


def _tap(arr, ox, oy):
    """arr at (y + oy, x + ox), indices clamped into the film (the caller masks what lies outside)."""
    h, w = arr.shape[:2]
    ys, xs = np.clip(np.arange(h) + oy, 0, h - 1), np.clip(np.arange(w) + ox, 0, w - 1)
    return arr[ys][:, xs]


def _inside(h, w, ox, oy):
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    return ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]


def np_variance(counts, stats):
    with np.errstate(all="ignore"):
        nd = counts.astype(np.float64)
        s1, s2 = stats[..., 0], stats[..., 1]
        num = nd * s2 - s1 * s1
        num = np.where(num < 0.0, 0.0, num)
        return (num / (nd * nd * (nd - 1.0))).astype(F)


def np_denoise(film, counts, stats, guides, iterations=5, sl=4.0, sz=1.0, a=7, extra_dead=None):
    """DESIGN.md section 13 in np.float32, in the rules header's order of operations: (film [H,W,4], variance [H,W]).  `extra_dead`: pixels treated as
    dead whatever they hold (their taps are skipped, they are copied through)."""
    film = np.asarray(film, F); guides = np.asarray(guides, F)
    h, w = counts.shape
    sl, sz = F(sl), F(sz)
    kern = [F(0.375), F(0.25), F(0.0625)]
    with np.errstate(all="ignore"):
        c = [film[..., k].copy() for k in range(3)]
        v = np_variance(counts, stats)
        dead = ~(np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & np.isfinite(v))
        if extra_dead is not None:
            dead = dead | extra_dead
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
            s = 1 << it
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
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx * s, dy * s
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
            c = [np.where(dead, c[k], sc[k] / sw) for k in range(3)]
            v = np.where(dead, v, sv / (sw * sw))
        out = np.zeros((h, w, 4), F)
        for k in range(3):
            out[..., k] = c[k]
        return out, v.astype(F)


def np_guides(sc, rd, K):
    """The fold of the two probes of `sc` (any library's scene): N += normal, Z += t over the valid hits in sample order, G = (N / K, Z / hits or 0)."""
    n = rd.width * rd.height
    px = np.arange(n, dtype=np.uint32)
    nsum, zsum, hits = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, np.uint32)
    for k in range(K):
        o, d, _ = sc.camera_samples(rd, px, np.full(n, k, np.uint32))
        h = sc.intersect(o, d)
        ok = h["valid"] != 0
        nsum = np.where(ok[:, None], nsum + h["normal"].astype(F), nsum)
        zsum = np.where(ok, zsum + h["t"].astype(F), zsum)
        hits = hits + ok.astype(np.uint32)
    g = np.zeros((n, 4), F)
    g[:, :3] = nsum / F(K)
    with np.errstate(all="ignore"):
        g[:, 3] = np.where(hits > 0, zsum / np.maximum(hits, 1).astype(F), F(0.0))
    return g.reshape(rd.height, rd.width, 4)


# ------------------------------------------------------------------------------------------------ inputs
SCENES = ("cornell_box", "cornell_gem", "mixed_primitives", "hdri_small")
GUIDE_SCENES = SCENES + ("panorama_test",)
BOUNCES = 6
_RENDERS = {}


def emulated_inputs(pkg, emu, name, w=48, h=48, spp=20, seed=1, K=4, **kw):
    """An emulated render of `name` with its statistics and guides (kept for the session: the exactness and the quality checks share them)."""
    key = (name, w, h, spp, seed, K, tuple(sorted(kw.items())))
    if key not in _RENDERS:
        sc = emu.create_scene(getattr(pkg.scene, name)())
        rd = pkg.api.render_desc(w, h, spp, BOUNCES, seed=seed, **kw)
        film, counts, st, _ = sc.render_adaptive(rd, spp, 0.0, stats=True)
        _RENDERS[key] = (film, counts, st, sc.render_guides(rd, K))
    return _RENDERS[key]


def synthetic_inputs(w, h, seed, dead=True):
    """Seeded inputs that meet every rule: three surfaces with their own normals and depth planes, a sky region, zero variances, outliers, and (with
    `dead`) pixels with NaN / infinite film values or statistics."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    region = (xx * 3 // max(w, 1) + (yy > h * 0.6).astype(int)) % 3
    normals = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])
    guides = np.zeros((h, w, 4), F)
    guides[..., :3] = (normals[region] + rng.normal(0.0, 0.02, (h, w, 3))).astype(F)
    guides[..., 3] = (2.0 + region + 0.01 * xx + 0.02 * yy + rng.normal(0.0, 0.001, (h, w))).astype(F)
    sky = (xx + yy) < min(w, h) * 0.35
    guides[sky] = 0.0
    base = np.array([0.2, 0.5, 0.9])[region] * (1.0 + 0.3 * np.sin(xx * 0.21) * np.cos(yy * 0.17))
    base = np.where(sky, 0.05 + 0.002 * yy, base)
    counts = rng.choice(np.array([2, 10, 20, 40, 64], np.uint32), (h, w))
    sigma = base * rng.choice([0.0, 0.05, 0.3], (h, w), p=[0.15, 0.6, 0.25])
    y = base + sigma / np.sqrt(counts) * rng.normal(0.0, 1.0, (h, w))
    fire = rng.random((h, w)) < 0.01
    y = np.where(fire, y * 20.0, y)
    film = np.zeros((h, w, 4), F)
    film[..., 0] = (0.9 * y).astype(F); film[..., 1] = y.astype(F); film[..., 2] = (1.1 * y + 0.01).astype(F)
    n = counts.astype(np.float64)
    s1 = n * film[..., 1].astype(np.float64)
    s2 = s1 * s1 / n + (n - 1.0) * (sigma * (1.0 + 4.0 * fire)) ** 2
    exact = sigma == 0.0   # S1 = n m and S2 = n m^2 with m a multiple of 1/64: n S2 - S1^2 is exactly 0
    m = np.round(film[..., 1].astype(np.float64) * 64.0) / 64.0
    s1 = np.where(exact, n * m, s1); s2 = np.where(exact, n * m * m, s2)
    stats = np.stack([s1, s2], -1)
    if dead:
        k = rng.random((h, w))
        film[k < 0.004, 1] = np.nan
        film[(k >= 0.004) & (k < 0.007), 0] = np.inf
        film[(k >= 0.007) & (k < 0.009), 2] = -np.inf
        stats[(k >= 0.009) & (k < 0.012), 1] = np.nan
        stats[(k >= 0.012) & (k < 0.014), 1] = np.inf
        film[0, 0, 1] = np.nan; film[h - 1, w - 1, 0] = np.inf   # (the corners too)
    return film, counts, np.ascontiguousarray(stats), guides


OFF_DEFAULT = dict(iterations=3, sigma_luminance=2.5, sigma_depth=0.5, normal_power_log2=3)


def np_kwargs(kw):
    return dict(iterations=kw.get("iterations", 5), sl=kw.get("sigma_luminance", 4.0), sz=kw.get("sigma_depth", 1.0), a=kw.get("normal_power_log2", 7))


def check_against_numpy(lib, inputs, **kw):
    film, counts, stats, guides = inputs
    got, gvar = lib.denoise_film(film, counts, stats, guides, variance=True, **kw)
    want, wvar = np_denoise(film, counts, stats, guides, **np_kwargs(kw))
    assert bits_equal(got, want), "film: %d values differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(gvar, wvar), "variance: %d values differ" % int((gvar.view(np.uint32) != wvar.view(np.uint32)).sum())
    assert np.all(got[..., 3] == 0.0)
    return got, gvar


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_the_entries_and_the_desc_mirrors_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    assert hasattr(lib, "pt_render_guides") and hasattr(lib, "pt_denoise_film")
    assert "denoise_film" not in pkg.api.API_FUNCTIONS and "render_guides" not in pkg.api.API_FUNCTIONS   # (pt_api.h's list: the boundary the oracle shares)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pt_denoise.h")).read(), flags=re.S)
    body = re.search(r"typedef struct pt_denoise_desc \{(.*?)\} pt_denoise_desc;", text, re.S).group(1)
    fields = []
    for decl in re.findall(r"(uint32_t|float)\s+([^;]+);", body):
        for name in decl[1].split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            fields.append((decl[0], m.group(1), int(m.group(2)) if m.group(2) else 0))
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t] * k if k else ctype[t]) for t, n, k in fields] == list(pkg.api.DenoiseDesc._fields_)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "pt_denoise.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(pt_denoise_desc)' + \
        "".join(", offsetof(pt_denoise_desc, %s)" % n for _, n, _ in fields) + "); return 0; }"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    D = pkg.api.DenoiseDesc
    assert out == [C.sizeof(D)] + [getattr(D, n).offset for _, n, _ in fields]


def _refusals(lib, prefix, last_error, sc, pkg, valid_status):
    """Every rule of include/pt_denoise.h's entries against one library; `valid_status`: what a valid call returns (PT_OK, or PT_ERR_NO_DEVICE)."""
    a = pkg.api
    W, H = 6, 5
    film, counts, stats, guides = synthetic_inputs(W, H, 3, dead=False)
    out, var = np.zeros((H, W, 4), F), np.zeros((H, W), F)
    den = getattr(lib, prefix + "denoise_film")
    den.restype = C.c_int32
    den.argtypes = [C.POINTER(a.DenoiseDesc), f32p, u32p, f64p, f32p, f32p, f32p]
    P = dict(film=film.ctypes.data_as(f32p), counts=counts.ctypes.data_as(u32p), stats=stats.ctypes.data_as(f64p), guides=guides.ctypes.data_as(f32p),
             out=out.ctypes.data_as(f32p), var=var.ctypes.data_as(f32p))

    def status(desc=None, null_desc=False, **over):
        p = dict(P); p.update(over)
        d = a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0) if desc is None else desc
        return den(None if null_desc else C.byref(d), p["film"], p["counts"], p["stats"], p["guides"], p["out"], p["var"])

    def desc(**kw):
        d = a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert status() == valid_status
    assert status(var=None) == valid_status          # (out_variance may be NULL)
    assert status(desc(iterations=10, normal_power_log2=10)) == valid_status
    assert status(null_desc=True) == PT_ERR_INVALID_ARGUMENT
    for name in ("film", "counts", "stats", "guides", "out"):
        assert status(**{name: None}) == PT_ERR_INVALID_ARGUMENT, name
    assert status(desc(width=0)) == PT_ERR_INVALID_ARGUMENT
    assert status(desc(height=0)) == PT_ERR_INVALID_ARGUMENT
    r = desc(); r.reserved[0] = 1
    assert status(r) == PT_ERR_INVALID_ARGUMENT
    assert b"reserved" in last_error()
    assert status(desc(iterations=11)) == PT_ERR_INVALID_ARGUMENT
    assert status(desc(normal_power_log2=11)) == PT_ERR_INVALID_ARGUMENT
    for field in ("sigma_luminance", "sigma_depth"):
        for bad in (-1.0, float("nan"), float("inf")):
            assert status(desc(**{field: bad})) == PT_ERR_INVALID_ARGUMENT, (field, bad)
    assert b"sigma_depth" in last_error()
    for bad in (0, 1):
        c2 = counts.copy(); c2[H - 1, W - 1] = bad
        assert status(counts=c2.ctypes.data_as(u32p)) == PT_ERR_INVALID_ARGUMENT
    assert b"sample count below 2" in last_error()
    g2 = guides.copy(); g2[2, 3, 3] = np.nan
    assert status(guides=g2.ctypes.data_as(f32p)) == PT_ERR_INVALID_ARGUMENT
    gd = getattr(lib, prefix + "render_guides")
    gd.restype = C.c_int32
    gd.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.c_uint32, f32p]
    rd = a.render_desc(W, H, 10, 3)
    assert gd(sc.handle, C.byref(rd), 2, P["guides"]) == valid_status
    assert gd(sc.handle, C.byref(rd), 0, P["guides"]) == PT_ERR_INVALID_ARGUMENT
    assert b"guide_samples" in last_error()
    assert gd(None, C.byref(rd), 2, P["guides"]) == PT_ERR_INVALID_ARGUMENT
    assert gd(sc.handle, None, 2, P["guides"]) == PT_ERR_INVALID_ARGUMENT
    assert gd(sc.handle, C.byref(rd), 2, None) == PT_ERR_INVALID_ARGUMENT
    assert gd(sc.handle, C.byref(a.render_desc(0, H, 10, 3)), 2, P["guides"]) == PT_ERR_INVALID_ARGUMENT
    assert gd(sc.handle, C.byref(a.render_desc(W, H, 10, 3, camera_index=7)), 2, P["guides"]) == PT_ERR_INVALID_ARGUMENT


def test_emulation_refuses_each_rule(emu_dn, pkg):
    err = emu_dn.lib.ptemu_denoise_last_error
    err.restype = C.c_char_p
    _refusals(emu_dn.lib, "ptemu_", err, emu_dn.create_scene(pkg.scene.cornell_box()), pkg, PT_OK)


def test_engine_checks_its_arguments_before_it_looks_for_a_device(pkg):
    """The engine's own entries, on any machine: pt_denoise_film takes no scene, so its refusals need no GPU; a valid call without a device is
    PT_ERR_NO_DEVICE (there is no CPU fallback)."""
    a = pkg.api
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_device_count.restype = C.c_uint32
    has_gpu = lib.pt_device_count() > 0
    W, H = 6, 5
    film, counts, stats, guides = synthetic_inputs(W, H, 3, dead=False)
    out = np.zeros((H, W, 4), F)
    den = lib.pt_denoise_film
    den.restype = C.c_int32
    den.argtypes = [C.POINTER(a.DenoiseDesc), f32p, u32p, f64p, f32p, f32p, f32p]
    args = (film.ctypes.data_as(f32p), counts.ctypes.data_as(u32p), stats.ctypes.data_as(f64p), guides.ctypes.data_as(f32p), out.ctypes.data_as(f32p), None)
    assert den(C.byref(a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0)), *args) == (PT_OK if has_gpu else PT_ERR_NO_DEVICE)
    if not has_gpu:
        assert b"no CPU fallback" in lib.pt_last_error()
    assert den(C.byref(a.DenoiseDesc(W, H, 11, 0.0, 0.0, 0, 0)), *args) == PT_ERR_INVALID_ARGUMENT
    assert b"iterations" in lib.pt_last_error()
    assert den(C.byref(a.DenoiseDesc(W, H, 0, -1.0, 0.0, 0, 0)), *args) == PT_ERR_INVALID_ARGUMENT
    assert den(C.byref(a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0)), None, *args[1:]) == PT_ERR_INVALID_ARGUMENT
    c2 = counts.copy(); c2[0, 0] = 1
    assert den(C.byref(a.DenoiseDesc(W, H, 0, 0.0, 0.0, 0, 0)), args[0], c2.ctypes.data_as(u32p), *args[2:]) == PT_ERR_INVALID_ARGUMENT
    assert b"sample count below 2" in lib.pt_last_error()
    gd = lib.pt_render_guides
    gd.restype = C.c_int32
    gd.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.c_uint32, f32p]
    assert gd(None, C.byref(a.render_desc(W, H, 10, 3)), 2, args[3]) == PT_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", GUIDE_SCENES)
def test_emulated_guides_equal_the_fold_of_the_oracles_probes(emu_dn, oracle, pkg, name):
    """ptemu_render_guides against the numpy fold of ptref_camera_samples + ptref_intersect, bit for bit, K = 1 and 4 (hdri_small and panorama_test
    have sky pixels: normal sum 0, distance 0)."""
    builder = getattr(pkg.scene, name)()
    rd = pkg.api.render_desc(40, 28, 10, 4, seed=5)
    esc, osc = emu_dn.create_scene(builder), oracle.create_scene(builder)
    for K in (1, 4):
        got, want = esc.render_guides(rd, K), np_guides(osc, rd, K)
        assert bits_equal(got, want), (name, K)
    if name in ("hdri_small", "panorama_test"):
        assert np.any(np.all(got[..., :3] == 0.0, -1) & (got[..., 3] == 0.0))
    assert np.any(got[..., 3] > 0.0)


def test_pt_exp_restatement_matches_the_header(emu_dn):
    """The numpy pt_exp against the header's, through the filter's own use of it: also checked directly on the arguments the filter can produce
    ([-80, 0]) with a C program compiled from include/pt_numerics.h."""
    x = np.concatenate([-np.linspace(0.0, 80.0, 4001), -np.random.default_rng(1).random(4000) * 80.0, [-80.0, -0.0, 0.0, -1e-30, -87.5, -104.0, 1.0, 89.0]]).astype(F)
    src = '#include <stdio.h>\n#include "pt_numerics.h"\nint main(void) { float x; while (fread(&x, 4, 1, stdin) == 1) { float r = pt_exp(x); fwrite(&r, 4, 1, stdout); } return 0; }'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = np.frombuffer(subprocess.run([os.path.join(d, "t")], input=x.tobytes(), capture_output=True, check=True).stdout, F)
    with np.errstate(all="ignore"):
        assert bits_equal(np_pt_exp(x), out)


@pytest.mark.parametrize("name", SCENES)
def test_filter_equals_the_numpy_restatement_on_emulated_renders(emu_dn, pkg, name):
    """48x48, 20 spp emulated renders with their own statistics and guides: film and variance bit for bit."""
    check_against_numpy(emu_dn, emulated_inputs(pkg, emu_dn, name))


def test_filter_equals_the_numpy_restatement_on_a_non_square_film(emu_dn, pkg):
    check_against_numpy(emu_dn, emulated_inputs(pkg, emu_dn, "mixed_primitives", w=70, h=45, spp=10, seed=4, K=2))


@pytest.mark.parametrize("w,h,seed,kw", [(64, 40, 11, {}), (37, 53, 12, OFF_DEFAULT), (5, 3, 13, dict(iterations=4)), (1, 9, 14, OFF_DEFAULT), (9, 1, 15, {}),
                                         (33, 17, 16, dict(iterations=10, normal_power_log2=10, sigma_luminance=0.25, sigma_depth=8.0))])
def test_filter_equals_the_numpy_restatement_on_synthetic_inputs(emu_dn, w, h, seed, kw):
    """Seeded inputs with sky regions, dead pixels (NaN / infinite film values and statistics), zero variances, and every desc field off its default."""
    inputs = synthetic_inputs(w, h, seed)
    got, _ = check_against_numpy(emu_dn, inputs, **kw)
    film = inputs[0]
    dead = ~np.isfinite(film[..., :3]).all(-1)
    assert bits_equal(got[dead][:, :3], film[dead][:, :3])       # a dead pixel is copied through ...
    alive = np.isfinite(film[..., :3]).all(-1) & np.isfinite(np_variance(inputs[1], inputs[2]))
    assert np.all(np.isfinite(got[alive]))                        # ... and never spreads


def _two_class_inputs(w, h, seed, right_guides, zero_right_variance):
    film, counts, stats, guides = synthetic_inputs(w, h, seed, dead=False)
    left = np.zeros((h, w), bool); left[:, : w // 2] = True
    guides[left] = (1.0, 0.0, 0.0, 3.0)
    guides[~left] = right_guides
    if zero_right_variance:
        n = counts.astype(np.float64)
        stats[~left, 0] = (n * 0.5)[~left]; stats[~left, 1] = (n * 0.25)[~left]   # (n S2 - S1^2 = 0 exactly)
    return film, counts, stats, guides, left


@pytest.mark.parametrize("right_guides", [(0.0, 1.0, 0.0, 3.0), (0.0, 0.0, 0.0, 0.0)], ids=["orthogonal_normals", "sky"])
def test_nothing_crosses_an_edge(emu_dn, right_guides):
    """Two half-planes with orthogonal normals, and surface against sky: changing the right half's film leaves the left half's output bit-identical.
    The film never crosses such an edge: every tap across it has weight 0 or is skipped.  What does cross, by the definition, is the 3x3 variance
    tent, which knows no geometry — and v_{i+1} of a right pixel depends on the right film through its weights.  So the statement is exact (a) for one
    pass with any statistics, and (b) for any number of passes when the right half's variances are 0 (they stay 0 whatever the film); both are
    asserted, and so is that the right half's statistics do not matter for one pass beyond the tent's one-pixel reach."""
    rng = np.random.default_rng(8)
    for zero_var, iterations in ((False, 1), (True, 5), (True, 10)):
        film, counts, stats, guides, left = _two_class_inputs(48, 40, 21, right_guides, zero_var)
        a = emu_dn.denoise_film(film, counts, stats, guides, iterations=iterations)
        film2 = film.copy()
        film2[~left, :3] = (film[~left, :3] * rng.uniform(0.0, 30.0, (int((~left).sum()), 3))).astype(F) + F(0.5)
        b = emu_dn.denoise_film(film2, counts, stats, guides, iterations=iterations)
        assert bits_equal(a[left], b[left]), (zero_var, iterations)
        assert not bits_equal(a[~left], b[~left])
    film, counts, stats, guides, left = _two_class_inputs(48, 40, 21, right_guides, False)
    a = emu_dn.denoise_film(film, counts, stats, guides, iterations=1)
    stats2 = stats.copy(); stats2[~left, 1] *= 3.0
    b = emu_dn.denoise_film(film, counts, stats2, guides, iterations=1)
    far = left.copy(); far[:, 48 // 2 - 3:] = False     # (the tent of p and of its taps at step 1 reach 3 pixels)
    assert bits_equal(a[far], b[far])


def test_a_dead_pixel_stays_one_pixel(emu_dn):
    """A NaN pixel comes out unchanged, and the output elsewhere equals that of the same input, the pixel finite, with the pixel's taps skipped."""
    film, counts, stats, guides = synthetic_inputs(40, 32, 31, dead=False)
    y, x = 13, 22
    guides[y, x] = guides[y, x + 1]   # (not sky: its neighbours would read it)
    mask = np.zeros((32, 40), bool); mask[y, x] = True
    for poison in ("film", "stats"):
        f2, s2 = film.copy(), stats.copy()
        if poison == "film":
            f2[y, x, 1] = np.nan
        else:
            s2[y, x, 1] = np.inf
        got, gvar = emu_dn.denoise_film(f2, counts, s2, guides, variance=True)
        want, wvar = np_denoise(film, counts, stats, guides, extra_dead=mask)
        assert bits_equal(got[~mask], want[~mask]) and bits_equal(gvar[~mask], wvar[~mask])
        assert bits_equal(got[y, x, :3], f2[y, x, :3])
        assert np.all(np.isfinite(got[~mask]))
        clean = emu_dn.denoise_film(film, counts, stats, guides)
        assert not bits_equal(got[~mask], clean[~mask])    # (the pixel did count before)


@pytest.mark.parametrize("iterations", [1, 5, 10])
def test_a_constant_film_stays_constant(emu_dn, iterations):
    """A constant film with arbitrary guides and variances returns the constant within I x 64 x 2^-24 relative (per pass: 25 products and 24 additions
    in the numerator, 24 additions in the weight sum, one division — at most 50 roundings of 2^-24 each)."""
    film, counts, stats, guides = synthetic_inputs(44, 36, 41, dead=False)
    const = np.array([0.7312, 1.9031, 0.0421], F)
    film[..., :3] = const
    out = emu_dn.denoise_film(film, counts, stats, guides, iterations=iterations)
    rel = np.abs(out[..., :3].astype(np.float64) - const.astype(np.float64)) / const.astype(np.float64)
    print("constant film, %d passes: largest relative deviation %.3g (bound %.3g)" % (iterations, rel.max(), iterations * 64 * 2.0 ** -24))
    assert rel.max() <= iterations * 64 * 2.0 ** -24


def film_rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


@pytest.mark.parametrize("name", SCENES)
def test_denoised_film_is_closer_to_a_converged_render(emu_dn, pkg, name):
    """The definition's quality, in the emulation: 48x48, 20 spp, seed 1, defaults, against a 1000-spp film of seed 77: the denoised film's RMSE over
    XYZ is below the noisy film's.  (The 1000-spp film's own noise puts a floor of about 0.14 under the ratio.)"""
    film, counts, st, guides = emulated_inputs(pkg, emu_dn, name)
    ref, _ = emu_dn.create_scene(getattr(pkg.scene, name)()).render(pkg.api.render_desc(48, 48, 1000, BOUNCES, seed=77))
    den = emu_dn.denoise_film(film, counts, st, guides)
    e0, e1 = film_rmse(film, ref), film_rmse(den, ref)
    print("%s: rmse noisy %.4g, denoised %.4g, ratio %.3f; mean Y %.5g -> %.5g (%+.1f %%)" %
          (name, e0, e1, e1 / e0, film[..., 1].mean(), den[..., 1].mean(), 100.0 * (den[..., 1].mean() / film[..., 1].mean() - 1.0)))
    assert e1 < e0


# ------------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("name", GUIDE_SCENES)
def test_gpu_guides_equal_the_emulation_and_the_fold_of_the_engines_probes(engine, emu_dn, pkg, name):
    builder = getattr(pkg.scene, name)()
    rd = pkg.api.render_desc(40, 28, 10, 4, seed=5)
    gsc, esc = engine.create_scene(builder), emu_dn.create_scene(builder)
    for K in (1, 4):
        got = gsc.render_guides(rd, K)
        assert bits_equal(got, esc.render_guides(rd, K)), (name, K)
        assert bits_equal(got, np_guides(gsc, rd, K)), (name, K)


def check_against_emulation(engine, emu, inputs, **kw):
    got, gvar = engine.denoise_film(*inputs, variance=True, **kw)
    want, wvar = emu.denoise_film(*inputs, variance=True, **kw)
    assert bits_equal(got, want), "film: %d values differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bits_equal(gvar, wvar), "variance: %d values differ" % int((gvar.view(np.uint32) != wvar.view(np.uint32)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("hero", [1, 4])
@pytest.mark.parametrize("name", SCENES)
def test_gpu_filter_equals_the_emulation_on_rendered_films(engine, emu_dn, pkg, name, hero):
    """The engine's own 48x48, 20-spp adaptive render (one and four wavelengths per path), statistics and guides through both filters."""
    sc = engine.create_scene(getattr(pkg.scene, name)())
    rd = pkg.api.render_desc(48, 48, 20, BOUNCES, seed=1, hero_wavelengths=hero)
    film, counts, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
    check_against_emulation(engine, emu_dn, (film, counts, st, sc.render_guides(rd, 4)))


@pytest.mark.gpu
def test_gpu_filter_equals_the_emulation_on_a_non_square_film(engine, emu_dn, pkg):
    sc = engine.create_scene(pkg.scene.mixed_primitives())
    rd = pkg.api.render_desc(70, 45, 10, BOUNCES, seed=4)
    film, counts, st, _ = sc.render_adaptive(rd, 10, 0.0, stats=True)
    check_against_emulation(engine, emu_dn, (film, counts, st, sc.render_guides(rd, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed,kw", [(64, 40, 11, {}), (37, 53, 12, OFF_DEFAULT), (5, 3, 13, dict(iterations=4)), (1, 9, 14, OFF_DEFAULT), (9, 1, 15, {}),
                                         (33, 17, 16, dict(iterations=10, normal_power_log2=10, sigma_luminance=0.25, sigma_depth=8.0))])
def test_gpu_filter_equals_the_emulation_on_synthetic_inputs(engine, emu_dn, w, h, seed, kw):
    check_against_emulation(engine, emu_dn, synthetic_inputs(w, h, seed), **kw)


def spread_rel(lib, builder, rd, q):
    """A relative error target between the pixels' own round-0 errors (their q-quantile), so that an adaptive render of `rd` spreads its counts."""
    _, _, st, _ = lib.create_scene(builder).render_adaptive(rd, rd.spp, 0.0, stats=True)
    n = float(rd.spp)
    s1, s2 = st[..., 0].ravel(), st[..., 1].ravel()
    ok = s1 > 0
    err = np.sqrt(np.maximum(n * s2[ok] - s1[ok] * s1[ok], 0.0) / (n - 1.0)) / s1[ok]
    return float(np.float32(np.quantile(err, q)))


@pytest.mark.gpu
def test_gpu_filter_equals_the_emulation_on_an_adaptive_render_with_spread_counts(engine, emu_dn, pkg):
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(64, 48, 10, 5, seed=7)
    rel = spread_rel(engine, builder, rd, 0.4)
    sc = engine.create_scene(builder)
    film, counts, st, _ = sc.render_adaptive(rd, 60, rel, step=10, stats=True)
    assert len(np.unique(counts)) >= 3, np.unique(counts)
    check_against_emulation(engine, emu_dn, (film, counts, st, sc.render_guides(rd, 4)))


@pytest.mark.gpu
def test_gpu_filter_equals_the_emulation_on_the_outputs_of_two_virtual_devices(engine, emu_dn, pkg):
    builder = pkg.scene.cornell_gem()
    rd = pkg.api.render_desc(64, 64, 10, 5, seed=3)
    rel = spread_rel(engine, builder, rd, 0.4)
    t = engine.tuning_default()
    t.multi_virtual = 2
    sc = engine.create_scene(builder, tuning=t)
    film, counts, st, _ = sc.render_adaptive_multi(rd, 40, rel, step=10, stats=True, device_mask=1)
    assert len(np.unique(counts)) >= 2
    check_against_emulation(engine, emu_dn, (film, counts, st, sc.render_guides(rd, 4)))


@pytest.mark.gpu
def test_gpu_filter_equals_the_emulation_at_1024(engine, emu_dn):
    """One seeded synthetic 1024x1024 input: tile edges, the wide steps across many workgroups."""
    check_against_emulation(engine, emu_dn, synthetic_inputs(1024, 1024, 51), iterations=6)


@pytest.mark.gpu
def test_gpu_render_denoised_equals_the_three_calls(engine, pkg):
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(64, 64, 20, 5, seed=2)
    sc = engine.create_scene(builder)
    film, den, counts, prof = sc.render_denoised(rd)
    f2, c2, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
    want = engine.denoise_film(f2, c2, st, sc.render_guides(rd, 4))
    assert bits_equal(film, f2) and np.array_equal(counts, c2) and bits_equal(den, want)
    assert prof.camera_rays == int(counts.sum()) and not bits_equal(den, film)
    film, den, counts, _ = sc.render_denoised(rd, max_samples=40, rel_error=0.05, guide_samples=2, iterations=3, sigma_luminance=2.0, device_mask=1)
    f2, c2, st, _ = sc.render_adaptive_multi(rd, 40, 0.05, stats=True, device_mask=1)
    want = engine.denoise_film(f2, c2, st, sc.render_guides(rd, 2), iterations=3, sigma_luminance=2.0)
    assert bits_equal(film, f2) and np.array_equal(counts, c2) and bits_equal(den, want)


def _read_png_rgba(path):
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big"); kind = data[pos + 4:pos + 8]; body = data[pos + 8:pos + 8 + n]; pos += 12 + n
        if kind == b"IHDR":
            w, h = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big")
            assert body[8:13] == bytes([8, 6, 0, 0, 0])
        elif kind == b"IDAT":
            idat += body
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w).astype(np.int32)
    out = np.zeros((h, w * 4), np.int32)
    prev = np.zeros(w * 4, np.int32)
    for y in range(h):
        ft, line = raw[y, 0], raw[y, 1:].copy()
        if ft == 1:
            for i in range(4, 4 * w):
                line[i] = (line[i] + line[i - 4]) & 255
        elif ft == 2:
            line = (line + prev) & 255
        else:
            assert ft == 0, "PNG filter %d is not handled by this reader" % ft
        out[y] = prev = line
    return out.reshape(h, w, 4).astype(np.uint8)


@pytest.mark.gpu
def test_gpu_ptcli_denoise(engine, pkg, tmp_path):
    """ptcli --denoise on config_cornell_c1.toml's settings at 64x64 with min_samples = 20: the two extra files hold pt_output_film of the API's denoised
    film, and the files written before are byte-identical to a run without the flag.  On config_cornell_c1.toml as it is (16 spp) the flag is refused
    with the adaptive path's message, a non-zero exit, and nothing written."""
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    text = open(os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c1.toml")).read()
    text = text.replace("min_samples = 16", "min_samples = 20").replace("width = 256", "width = 64").replace("height = 256", "height = 64")
    assert "min_samples = 20" in text and "width = 64" in text and "height = 64" in text
    cfg = tmp_path / "config.toml"
    cfg.write_text(text)
    runs = {}
    for tag, extra in (("plain", []), ("denoise", ["--denoise"])):
        out = tmp_path / tag
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(out), "--write-film", "--seed", "5"] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = out
    assert sorted(os.listdir(runs["plain"])) == ["beauty.exr", "beauty.npy", "beauty.png"]
    assert sorted(os.listdir(runs["denoise"])) == ["beauty.exr", "beauty.npy", "beauty.png", "beauty_denoised.exr", "beauty_denoised.npy", "beauty_denoised.png"]
    for f in ("beauty.exr", "beauty.npy", "beauty.png"):
        assert open(runs["plain"] / f, "rb").read() == open(runs["denoise"] / f, "rb").read(), f
    # the API's denoised film of the same settings
    sf = pkg.scene_file
    config = sf.Config(str(cfg))
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    film, den, _, _ = sc.render_denoised(config.render_desc(0, seed=5))
    assert bits_equal(np.load(runs["denoise"] / "beauty.npy"), film) and bits_equal(np.load(runs["denoise"] / "beauty_denoised.npy"), den)
    assert not bits_equal(film, den)
    od = config.output_desc(0)
    rgba = np.zeros((64, 64, 4), np.uint8)
    linear = np.zeros((64, 64, 3), F)
    engine.check(engine._output_film(C.byref(od), den.ctypes.data_as(f32p), rgba.ctypes.data_as(C.POINTER(C.c_uint8)), linear.ctypes.data_as(f32p)))
    assert np.array_equal(_read_png_rgba(str(runs["denoise"] / "beauty_denoised.png")), rgba)
    exr = sf.read_image(str(runs["denoise"] / "beauty_denoised.exr"), sf.IMAGE_EXR, alpha_fill=1.0)
    assert bits_equal(exr[..., :3], linear)
    # as it is: 16 spp
    out = tmp_path / "refused"
    r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c1.toml"), "--output-dir", str(out), "--denoise"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=180)
    assert r.returncode != 0
    assert "multiples of 10" in r.stderr and "--denoise" in r.stderr
    assert "rendering" not in r.stdout
    assert not out.exists() or os.listdir(out) == []
