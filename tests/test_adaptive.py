"""Adaptive sampling between min_samples and max_samples (include/pt_adaptive.h).  Every pixel of an adaptive render is, bit for
bit, that pixel of a fixed render at the pixel's own count, so the checks are exact: the CPU tier compares the per-round decision and compaction with a
numpy restatement and the emulation's driver with a numpy driver built from one-sample films; the GPU tier compares the engine with the emulation and
with its own pt_render."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED, PT_OK

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)


@pytest.fixture(scope="session")
def emu_ad(pkg):
    """The host emulation (tests/host_emulation/ptemu.cpp) with the adaptive driver (ptemu_adaptive.cpp) beside it: a library of its own."""
    emu = emulation.load(pkg, "adaptive")
    sel = emu.lib.ptemu_adaptive_select
    sel.restype = C.c_int32
    sel.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint32, f64p, C.c_uint32, C.c_float, C.c_float, u32p, C.POINTER(C.c_uint8), u32p, u32p]
    return emu


# ------------------------------------------------------------------------------------------------ numpy restatement of the definition
def np_unconverged(n, s1, s2, rel, abs_):
    """NOT (n*S2 - S1*S1 <= (n-1)*M*M), M = max(rel*S1, abs*n), in f64 (rel and abs are the f32 values of the desc)."""
    with np.errstate(all="ignore"):
        nd = np.float64(n)
        a = np.float64(np.float32(rel)) * s1
        b = np.float64(np.float32(abs_)) * nd
        m = np.where(a > b, a, b)
        lhs = nd * s2 - s1 * s1
        rhs = (nd - 1.0) * m * m
        return ~(lhs <= rhs)


def np_dilate(img):
    """3x3 neighbourhood OR inside the film."""
    h, w = img.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = img
    out = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def np_select(w, h, lst, count, stats, max_samples, rel, abs_):
    """One round: the unconverged byte image and the next list (in the order of `lst`)."""
    unc = np.zeros(w * h, np.uint8)
    unc[lst] = np_unconverged(count, stats[lst, 0], stats[lst, 1], rel, abs_)
    keep = np_dilate(unc.reshape(h, w) != 0).ravel()[lst] & (count < max_samples)
    return unc, lst[keep]


def emu_select(emu, w, h, lst, count, stats, max_samples, rel, abs_):
    lst = np.ascontiguousarray(lst, np.uint32)
    stats = np.ascontiguousarray(stats, np.float64)
    counts = np.full(w * h, 7, np.uint32)
    unc = np.full(w * h, 99, np.uint8)
    nxt = np.zeros(max(len(lst), 1), np.uint32)
    nn = C.c_uint32(0)
    st = emu.lib.ptemu_adaptive_select(w, h, lst.ctypes.data_as(u32p), len(lst), count, stats.ctypes.data_as(f64p), max_samples, rel, abs_,
                                       counts.ctypes.data_as(u32p), unc.ctypes.data_as(C.POINTER(C.c_uint8)), nxt.ctypes.data_as(u32p), C.byref(nn))
    assert st == PT_OK
    return counts, unc, nxt[:nn.value]


def pick_rel(lib, builder, rd, q):
    """A relative error target between the pixels' own round-0 errors (their q-quantile), so that an adaptive render of `rd` spreads its counts."""
    sc = lib.create_scene(builder)
    _, _, st, _ = sc.render_adaptive(rd, rd.spp, 0.0, stats=True)
    n = float(rd.spp)
    s1, s2 = st[..., 0].ravel(), st[..., 1].ravel()
    ok = s1 > 0
    err = np.sqrt(np.maximum(n * s2[ok] - s1[ok] * s1[ok], 0.0) / (n - 1.0)) / s1[ok]
    return float(np.float32(np.quantile(err, q)))


def np_adaptive_driver(ones, w, h, spp, step, max_samples, rel, abs_=0.0):
    """The definition, driven in numpy over one-sample films ones[s] (H, W, 4): film, counts, stats."""
    npx = w * h
    total = np.zeros((npx, 3), np.float32)
    phase = np.zeros((npx, 3), np.float32)
    s1 = np.zeros(npx, np.float64)
    s2 = np.zeros(npx, np.float64)
    counts = np.zeros(npx, np.uint32)
    active = np.ones(npx, bool)
    c, ln, rounds = 0, spp, 0
    while True:
        idx = np.nonzero(active)[0]
        for s in range(c, c + ln):
            o = ones[s].reshape(-1, 4)
            phase[idx] = phase[idx] + o[idx, :3]
            y = o[idx, 1].astype(np.float64)
            s1[idx] += y
            s2[idx] += y * y
            if (s + 1) % 10 == 0:
                total[idx] = total[idx] + phase[idx]
                phase[idx] = 0.0
        c += ln
        rounds += 1
        counts[idx] = c
        if c >= max_samples:
            break
        unc = np.zeros(npx, bool)
        unc[idx] = np_unconverged(c, s1[idx], s2[idx], rel, abs_)
        active = active & np_dilate(unc.reshape(h, w)).ravel()
        if not active.any():
            break
        ln = min(step, max_samples - c)
    film = np.zeros((npx, 4), np.float32)
    film[:, :3] = total / counts.astype(np.float32)[:, None]
    return film.reshape(h, w, 4), counts.reshape(h, w), np.stack([s1, s2], -1).reshape(h, w, 2), rounds


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_render_adaptive_and_the_desc_mirrors_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    assert hasattr(lib, "pt_render_adaptive")
    assert "render_adaptive" not in pkg.api.API_FUNCTIONS   # (pt_api.h's list: the boundary the oracle shares)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pt_adaptive.h")).read(), flags=re.S)
    body = re.search(r"typedef struct pt_adaptive_desc \{(.*?)\} pt_adaptive_desc;", text, re.S).group(1)
    fields = re.findall(r"(uint32_t|float)\s+(\w+);", body)
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(pkg.api.AdaptiveDesc._fields_)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "pt_adaptive.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(pt_adaptive_desc)' + \
        "".join(", offsetof(pt_adaptive_desc, %s)" % n for _, n in fields) + "); return 0; }"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    A = pkg.api.AdaptiveDesc
    assert out == [C.sizeof(A)] + [getattr(A, n).offset for _, n in fields]


@pytest.mark.parametrize("w,h", [(13, 7), (1, 9), (9, 1), (32, 20), (5, 5)])
def test_select_matches_the_numpy_restatement(emu_ad, w, h):
    """Decision, dilation and stable compaction of one round against numpy, bit for bit and in list order: random and constructed statistics (0,
    negative, NaN, infinite, exactly at the threshold), the film's borders and corners, lists in shuffled order, pixels at max_samples."""
    rng = np.random.default_rng(w * 100 + h)
    npx = w * h
    for trial in range(12):
        count = int(rng.choice([10, 20, 30, 60]))
        # realistic statistics: S1 = n * mean, S2 = n * (mean^2 + var)
        mean = rng.exponential(1.0, npx)
        var = mean * mean * rng.exponential(0.05, npx)
        stats = np.stack([count * mean, count * (mean * mean + var)], -1)
        special = rng.random(npx)
        stats[special < 0.05] = 0.0
        stats[(special >= 0.05) & (special < 0.08), 0] = -np.abs(stats[(special >= 0.05) & (special < 0.08), 0])
        stats[(special >= 0.08) & (special < 0.1), 1] = np.nan
        stats[(special >= 0.1) & (special < 0.11), 0] = np.inf
        # the threshold itself: n = 10, S1 = 20, S2 = 62.5, rel 0.25 -> n*S2 - S1^2 = 225 = (n-1)*(0.25*S1)^2 exactly
        rel = float(rng.choice([0.0, 0.05, 0.25, 1.0]))
        abs_ = float(rng.choice([0.0, 0.0, 0.01, 0.3]))
        if trial % 3 == 0:
            count, rel, abs_ = 10, 0.25, 0.0
            at = rng.random(npx) < 0.3
            stats[at] = (20.0, 62.5)
            stats[rng.random(npx) < 0.1] = (20.0, np.nextafter(62.5, 100.0))
        corners = np.array([0, w - 1, (h - 1) * w, npx - 1], np.uint32)
        lst = np.unique(np.concatenate([corners, rng.choice(npx, size=max(1, npx // 2), replace=False)])).astype(np.uint32)
        rng.shuffle(lst)
        for max_samples in (count + 10, count):   # (count == max_samples: the list ends)
            counts, unc, nxt = emu_select(emu_ad, w, h, lst, count, stats, max_samples, rel, abs_)
            want_unc, want_next = np_select(w, h, lst, count, stats, max_samples, rel, abs_)
            assert np.array_equal(unc, want_unc)
            assert np.array_equal(nxt, want_next)
            assert np.all(counts[lst] == count) and np.all(np.delete(counts, lst) == 7)
            if max_samples == count:
                assert len(nxt) == 0
        if trial % 3 == 0:
            # the exact threshold is converged, one ulp of S2 above is not
            u = want_unc[lst]
            at_thr = (stats[lst, 0] == 20.0) & (stats[lst, 1] == 62.5)
            above = (stats[lst, 0] == 20.0) & (stats[lst, 1] == np.nextafter(62.5, 100.0))
            assert np.all(u[at_thr] == 0) and np.all(u[above] == 1)


def test_validation_rejects_each_rule(emu_ad, pkg):
    a = pkg.api
    sc = emu_ad.create_scene(pkg.scene.cornell_box())

    def status(rd, max_samples=30, step=0, rel=0.1, abs_=0.0, counts=True):
        film = np.zeros((rd.height, rd.width, 4), np.float32)
        cnt = np.zeros((rd.height, rd.width), np.uint32)
        ad = a.AdaptiveDesc(max_samples, step, rel, abs_)
        return emu_ad.lib.ptemu_render_adaptive(sc.handle, C.byref(rd), C.byref(ad), film.ctypes.data_as(C.POINTER(C.c_float)),
                                                cnt.ctypes.data_as(u32p) if counts else None, None, None)

    emu_ad.lib.ptemu_render_adaptive.restype = C.c_int32
    emu_ad.lib.ptemu_render_adaptive.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(C.c_float), u32p, f64p, C.POINTER(a.Profile)]
    rd = lambda **k: a.render_desc(8, 8, k.pop("spp", 10), 3, **k)
    assert status(rd(), max_samples=10) == PT_OK          # max_samples == spp: one fixed render
    assert status(rd(), counts=False) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(phase_samples=20, spp=20)) == PT_ERR_UNSUPPORTED   # the Naive renderer's single phase
    assert status(rd(phase_samples=5)) == PT_ERR_UNSUPPORTED
    assert status(rd(phase_samples=10)) == PT_OK
    assert status(rd(shard=(0, 2))) == PT_ERR_UNSUPPORTED
    assert status(rd(first_sample=10, sample_count=10, spp=20)) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(sample_count=10)) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(spp=15)) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(), step=15) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(), max_samples=35) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(spp=40), max_samples=30) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(), rel=-0.1) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(), rel=float("nan")) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(), abs_=-1.0) == PT_ERR_INVALID_ARGUMENT
    assert status(rd(spp=0), max_samples=0) == PT_ERR_INVALID_ARGUMENT
    msg = emu_ad.lib.ptemu_adaptive_last_error
    msg.restype = C.c_char_p
    status(rd(spp=40), max_samples=30)
    assert b"max_samples" in msg()


def test_emulated_adaptive_render_equals_the_numpy_driver_and_fixed_renders(emu_ad, pkg):
    """16x16 Cornell box, spp 10, step 10, max_samples 60: film, counts and stats of ptemu_render_adaptive equal a numpy driver over one-sample
    ptemu_render films bit for bit, and every pixel equals ptemu_render at spp = its count."""
    a = pkg.api
    W = H = 16
    spp, step, mx = 10, 10, 60
    builder = pkg.scene.cornell_box()
    rd = a.render_desc(W, H, spp, 4, seed=3)
    rel = pick_rel(emu_ad, builder, rd, 0.35)
    sc = emu_ad.create_scene(builder)
    film, counts, stats, prof = sc.render_adaptive(rd, mx, rel, step=step, stats=True)
    assert len(np.unique(counts)) >= 3, np.unique(counts)
    assert prof.camera_rays == int(counts.sum())
    ones = [sc.render(a.render_desc(W, H, mx, 4, seed=3, first_sample=s, sample_count=1))[0] for s in range(mx)]
    nfilm, ncounts, nstats, rounds = np_adaptive_driver(ones, W, H, spp, step, mx, rel)
    assert np.array_equal(counts, ncounts)
    assert np.array_equal(stats.view(np.uint64), nstats.view(np.uint64))
    assert np.array_equal(film.view(np.uint32), nfilm.view(np.uint32))
    assert prof.kernel_launches[5] == rounds
    for n in np.unique(counts):
        fixed, _ = sc.render(a.render_desc(W, H, int(n), 4, seed=3))
        m = counts == n
        assert np.array_equal(film[m].view(np.uint32), fixed[m].view(np.uint32)), n


# ------------------------------------------------------------------------------------------------ GPU tier
def _five_scenes(pkg):
    a = pkg.api
    return {
        "cornell": (pkg.scene.cornell_box, dict()),
        "gem": (pkg.scene.cornell_gem, dict()),
        "hdri": (pkg.scene.hdri_small, dict()),
        "cornell_hero": (pkg.scene.cornell_box, dict(hero_wavelengths=4)),
        "fog_medium": (pkg.scene.fog_ball, dict(medium_aware=True)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell", "gem", "hdri", "cornell_hero", "fog_medium"])
def test_gpu_adaptive_equals_the_emulation(engine, emu_ad, pkg, case):
    """pt_render_adaptive on the GPU equals ptemu_render_adaptive bit for bit (film, counts, stats): one scene per kernel family."""
    make, kw = _five_scenes(pkg)[case]
    builder = make()
    rd = pkg.api.render_desc(16, 12, 10, 5, seed=7, **kw)
    rel = pick_rel(engine, builder, rd, 0.4)
    g = engine.create_scene(builder).render_adaptive(rd, 40, rel, step=10, stats=True)
    e = emu_ad.create_scene(builder).render_adaptive(rd, 40, rel, step=10, stats=True)
    assert len(np.unique(g[1])) >= 2, np.unique(g[1])
    assert np.array_equal(g[1], e[1])
    assert np.array_equal(g[2].view(np.uint64), e[2].view(np.uint64))
    assert np.array_equal(g[0].view(np.uint32), e[0].view(np.uint32))
    assert g[3].camera_rays == e[3].camera_rays == int(g[1].sum()) and g[3].kernel_launches[5] == e[3].kernel_launches[5]


@pytest.mark.gpu
def test_gpu_every_pixel_equals_pt_render_at_its_count(engine, pkg):
    """Cornell 128x128, spp 20, step 20, max_samples 200: every pixel equals the engine's own pt_render at spp = its count, bit for bit."""
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(128, 128, 20, 5, seed=11)
    rel = pick_rel(engine, builder, rd, 0.3)
    sc = engine.create_scene(builder)
    film, counts, prof = sc.render_adaptive(rd, 200, rel, step=20)
    levels = np.unique(counts)
    assert len(levels) >= 3, levels
    assert prof.camera_rays == int(counts.sum())
    for n in levels:
        fixed, _ = sc.render(pkg.api.render_desc(128, 128, int(n), 5, seed=11))
        m = counts == n
        assert np.array_equal(film[m].view(np.uint32), fixed[m].view(np.uint32)), n


@pytest.mark.gpu
def test_gpu_extreme_targets_are_fixed_renders(engine, pkg):
    """rel_error 0: every pixel runs to max_samples (the film is pt_render's at max_samples); a huge rel_error: every pixel stops at spp."""
    sc = engine.create_scene(pkg.scene.cornell_box())
    rd = pkg.api.render_desc(32, 32, 10, 5, seed=5)
    film, counts, prof = sc.render_adaptive(rd, 40, 0.0)
    assert np.all(counts == 40) and prof.kernel_launches[5] == 4
    fixed, _ = sc.render(pkg.api.render_desc(32, 32, 40, 5, seed=5))
    assert np.array_equal(film.view(np.uint32), fixed.view(np.uint32))
    film, counts, prof = sc.render_adaptive(rd, 40, 1e30)
    assert np.all(counts == 10) and prof.kernel_launches[5] == 1
    fixed, _ = sc.render(rd)
    assert np.array_equal(film.view(np.uint32), fixed.view(np.uint32))


@pytest.mark.gpu
def test_gpu_many_passes_per_round_change_nothing(engine, pkg):
    """batch_slots 4096 (rounds split into many passes) gives the default's outputs; profile.camera_rays is the sum of the counts."""
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(48, 40, 10, 5, seed=9)
    rel = pick_rel(engine, builder, rd, 0.4)
    ref = engine.create_scene(builder).render_adaptive(rd, 50, rel, step=20, stats=True)
    t = engine.tuning_default()
    t.batch_slots = 4096
    got = engine.create_scene(builder, tuning=t).render_adaptive(rd, 50, rel, step=20, stats=True)
    assert len(np.unique(ref[1])) >= 2
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64))
    assert got[3].camera_rays == ref[3].camera_rays == int(ref[1].sum())
    assert got[3].kernel_launches[0] > ref[3].kernel_launches[0]   # (more generate launches: more passes)


ADAPTIVE_CONFIG = """default_scene_file = "data/scenes/mixed_primitives.toml"

[renderer]
type = "Tiled"
tile_size = [16, 16]

[[render_settings]]
filename = "adaptive"
min_samples = 8
max_samples = 35
max_bounces = 4
hwss = false
camera_id = "main"
[render_settings.tonemap_settings]
type = "Clamp"
luminance_only = true
silenced = true
[render_settings.colorspace_settings]
type = "sRGB"
[render_settings.integrator]
type = "PT"
light_samples = 1
medium_aware = false
[render_settings.resolution]
width = 48
height = 32

[[render_settings]]
filename = "fixed"
min_samples = 10
max_bounces = 3
hwss = false
camera_id = "main"
[render_settings.tonemap_settings]
type = "Clamp"
luminance_only = true
silenced = true
[render_settings.colorspace_settings]
type = "sRGB"
[render_settings.integrator]
type = "PT"
light_samples = 1
medium_aware = false
[render_settings.resolution]
width = 32
height = 32
"""


@pytest.mark.gpu
def test_gpu_ptcli_adaptive(pkg, tmp_path):
    """ptcli --adaptive: the setting with max_samples renders 10..40 spp adaptively (rounded up, with a warning) and prints the summary; the one
    without renders as before, with a warning.  Both write their files."""
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    cfg = tmp_path / "config.toml"
    cfg.write_text(ADAPTIVE_CONFIG)
    out = tmp_path / "out"
    r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(out), "--adaptive", "0.05", "--write-film"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rounded up to 10..40" in r.stderr and "no max_samples > min_samples" in r.stderr
    m = re.search(r"adaptive: ([0-9.]+) samples per pixel on average, min (\d+), max (\d+), (\d+) rounds", r.stdout)
    assert m, r.stdout
    mean, lo, hi, rounds = float(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))
    assert 10 <= lo <= mean <= hi <= 40 and 1 <= rounds <= 4
    assert "rendering 32x32, 10 spp" in r.stdout and "render done" in r.stdout
    for name in ("adaptive", "fixed"):
        for ext in ("exr", "png", "npy"):
            assert (out / ("%s.%s" % (name, ext))).stat().st_size > 0
    film = np.load(out / "adaptive.npy")
    assert film.shape == (32, 48, 4) and np.all(np.isfinite(film)) and np.all(film[..., 3] == 0.0)
