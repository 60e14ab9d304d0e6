"""Adaptive sampling on every device of a node (pt_render_adaptive_multi, include/pt_adaptive.h).  The devices own disjoint
tile shards and run the rounds in lockstep, merging their unconverged images after every round, so the outputs are pt_render_adaptive's bit for bit.
The CPU tier checks the protocol in the host emulation (ptemu_adaptive_multi.cpp) against the one-device driver, and that the exchange matters; the GPU
tier checks the engine with virtual devices, plain masks, refusals and ptcli against pt_render_adaptive."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import emulation
from test_adaptive import ADAPTIVE_CONFIG, np_dilate, np_unconverged, pick_rel
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED, PT_OK

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
W, H = 77, 45   # 2 x 1 whole 32 x 32 tiles and remnant tiles on the right, at the bottom and in the corner: 6 tiles


@pytest.fixture(scope="session")
def emu_am(pkg):
    """The host emulation with the one-device adaptive driver and the sharded one beside it: a library of its own."""
    emu = emulation.load(pkg, "adaptive_multi")
    a = pkg.api
    fn = emu.lib.ptemu_render_adaptive_multi
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.c_uint32, C.POINTER(C.c_float), u32p, f64p, C.POINTER(a.Profile)]
    emu.lib.ptemu_adaptive_multi_last_error.restype = C.c_char_p
    return emu


def emu_multi(pkg, emu, sc, rd, shard_count, max_samples, rel, step=0, abs_=0.0, counts=True):
    """ptemu_render_adaptive_multi: (status, film, counts, stats, profile)"""
    film = np.zeros((rd.height, rd.width, 4), np.float32)
    cnt = np.zeros((rd.height, rd.width), np.uint32)
    st = np.zeros((rd.height, rd.width, 2), np.float64)
    prof = pkg.api.Profile()
    ad = pkg.api.AdaptiveDesc(max_samples, step, rel, abs_)
    s = emu.lib.ptemu_render_adaptive_multi(sc.handle, C.byref(rd), C.byref(ad), shard_count, film.ctypes.data_as(C.POINTER(C.c_float)),
                                            cnt.ctypes.data_as(u32p) if counts else None, st.ctypes.data_as(f64p), C.byref(prof))
    return s, film, cnt, st, prof


def np_owner(w, h, tw, th, n):
    """The shard of every pixel: the tiles in shard_pixels' order (whole tiles, the right column, the bottom row, the corner), tile t to PT_TILE_SHARD."""
    fx, fy, rx, ry = w // tw, h // th, w % tw, h % th
    tiles = [(x * tw, x * tw + tw, y * th, y * th + th) for y in range(fy) for x in range(fx)]
    if rx:
        tiles += [(fx * tw, w, y * th, y * th + th) for y in range(fy)]
    if ry:
        tiles += [(x * tw, x * tw + tw, fy * th, h) for x in range(fx)]
        if rx:
            tiles.append((fx * tw, w, fy * th, h))
    owner = np.full((h, w), -1, np.int64)
    for t, (x0, x1, y0, y1) in enumerate(tiles):
        owner[y0:y1, x0:x1] = (t + t // max(fx, 1)) % n
    assert (owner >= 0).all()
    return owner.ravel()


def np_sharded_counts(ones, w, h, owner, n, spp, step, max_samples, rel, exchange):
    """The counts of a sharded driver in numpy over one-sample films: every shard marks its own pixels; with `exchange` every shard dilates the merged
    image (the protocol), without it only its own image (what a device that never hears from the others would do)."""
    npx = w * h
    s1, s2 = np.zeros(npx), np.zeros(npx)
    counts = np.zeros(npx, np.uint32)
    active = np.ones(npx, bool)
    c, ln = 0, spp
    while True:
        idx = np.nonzero(active)[0]
        for s in range(c, c + ln):
            y = ones[s].reshape(-1, 4)[idx, 1].astype(np.float64)
            s1[idx] += y
            s2[idx] += y * y
        c += ln
        counts[idx] = c
        if c >= max_samples:
            break
        unc = np.zeros(npx, bool)
        unc[idx] = np_unconverged(c, s1[idx], s2[idx], rel, 0.0)
        if exchange:
            keep = np_dilate(unc.reshape(h, w)).ravel()
        else:
            keep = np.zeros(npx, bool)
            for k in range(n):
                keep |= np_dilate((unc & (owner == k)).reshape(h, w)).ravel() & (owner == k)
        active &= keep
        if not active.any():
            break
        ln = min(step, max_samples - c)
    return counts.reshape(h, w)


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_render_adaptive_multi_and_the_binding_mirrors_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    assert hasattr(lib, "pt_render_adaptive_multi")
    assert "render_adaptive_multi" not in pkg.api.API_FUNCTIONS   # (pt_adaptive.h, not the oracle's boundary)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pt_adaptive.h")).read(), flags=re.S)
    params = re.search(r"pt_status\s+pt_render_adaptive_multi\s*\((.*?)\);", text, re.S).group(1)
    types = [re.sub(r"\s+", " ", p.strip().rsplit(" ", 1)[0].replace("*", " *")).replace(" *", "*") for p in params.split(",")]
    assert types == ["pt_scene*", "const pt_render_desc*", "const pt_adaptive_desc*", "uint64_t", "float*", "uint32_t*", "double*", "pt_profile*"]
    a = pkg.api
    want = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint32),
            C.POINTER(C.c_double), C.POINTER(a.Profile)]
    fn = a.Library(pkg.LIBRARY_PATH)._render_adaptive_multi
    assert fn is not None and list(fn.argtypes) == want and fn.restype == C.c_int32
    # the Python method: render_adaptive's parameters, then the mask
    single = list(inspect.signature(a.Scene.render_adaptive).parameters)
    multi = list(inspect.signature(a.Scene.render_adaptive_multi).parameters)
    assert multi == single + ["device_mask"]
    assert inspect.signature(a.Scene.render_adaptive_multi).parameters["device_mask"].default == 0


SCENES = {
    "cornell": ("cornell_box", dict()),
    "gem": ("cornell_gem", dict()),
    "cornell_hero": ("cornell_box", dict(hero_wavelengths=4)),
}


@pytest.mark.parametrize("case", list(SCENES))
def test_emulated_sharded_driver_equals_the_one_device_driver(emu_am, pkg, case):
    """ptemu_render_adaptive_multi with 1, 2, 3, 4 and 8 shards of a 77 x 45 film equals ptemu_render_adaptive bit for bit: film as u32, counts,
    stats as u64, rounds and camera rays.  With 8 shards and 6 tiles two devices have nothing to render and take part all the same."""
    scene, kw = SCENES[case]
    builder = pkg.scene.SCENES[scene]()
    rd = pkg.api.render_desc(W, H, 10, 4, seed=7, **kw)
    rel = pick_rel(emu_am, builder, rd, 0.4)
    sc = emu_am.create_scene(builder)
    film, counts, stats, prof = sc.render_adaptive(rd, 40, rel, step=10, stats=True)
    assert counts.min() < counts.max(), np.unique(counts)
    for n in (1, 2, 3, 4, 8):
        s, mfilm, mcounts, mstats, mprof = emu_multi(pkg, emu_am, sc, rd, n, 40, rel, step=10)
        assert s == PT_OK
        assert np.array_equal(mcounts, counts), n
        assert np.array_equal(mstats.view(np.uint64), stats.view(np.uint64)), n
        assert np.array_equal(mfilm.view(np.uint32), film.view(np.uint32)), n
        assert mprof.kernel_launches[5] == prof.kernel_launches[5] and mprof.camera_rays == prof.camera_rays == int(counts.sum()), n


def test_the_exchange_is_what_makes_the_shards_agree(emu_am, pkg):
    """Not vacuous: a numpy sharded driver with the exchange gives the emulation's counts, and the same driver in which each shard dilates only its own
    image gives other counts — the pixels at the shard edges whose unconverged neighbours belong to another device."""
    a = pkg.api
    builder = pkg.scene.cornell_box()
    rd = a.render_desc(W, H, 10, 4, seed=7)
    rel = pick_rel(emu_am, builder, rd, 0.4)
    sc = emu_am.create_scene(builder)
    mx = 40
    ones = [sc.render(a.render_desc(W, H, mx, 4, seed=7, first_sample=s, sample_count=1))[0] for s in range(mx)]
    for n in (2, 4):
        owner = np_owner(W, H, 32, 32, n)
        _, _, counts, _, _ = emu_multi(pkg, emu_am, sc, rd, n, mx, rel, step=10)
        assert counts.min() < counts.max()
        assert np.array_equal(np_sharded_counts(ones, W, H, owner, n, 10, 10, mx, rel, exchange=True), counts), n
        isolated = np_sharded_counts(ones, W, H, owner, n, 10, 10, mx, rel, exchange=False)
        assert not np.array_equal(isolated, counts), n
        assert (isolated <= counts).all()   # (without the exchange a shard only ever stops earlier)


def test_emulated_sharded_driver_validation(emu_am, pkg):
    """The sharded driver takes normalize_adaptive_desc's checks unchanged, and needs at least one device."""
    a = pkg.api
    sc = emu_am.create_scene(pkg.scene.cornell_box())
    rd = lambda **k: a.render_desc(8, 8, k.pop("spp", 10), 3, **k)
    st = lambda r, n=2, **k: emu_multi(pkg, emu_am, sc, r, n, k.pop("max_samples", 30), k.pop("rel", 0.1), **k)[0]
    assert st(rd()) == PT_OK
    assert st(rd(), n=0) == PT_ERR_INVALID_ARGUMENT
    assert st(rd(), counts=False) == PT_ERR_INVALID_ARGUMENT
    assert st(rd(shard=(0, 2))) == PT_ERR_UNSUPPORTED
    assert st(rd(phase_samples=20, spp=20)) == PT_ERR_UNSUPPORTED
    assert st(rd(spp=15)) == PT_ERR_INVALID_ARGUMENT
    assert st(rd(), step=15) == PT_ERR_INVALID_ARGUMENT
    assert st(rd(spp=40), max_samples=30) == PT_ERR_INVALID_ARGUMENT
    assert b"max_samples" in emu_am.lib.ptemu_adaptive_multi_last_error()
    assert st(rd(), rel=float("nan")) == PT_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ GPU tier
GPU_SCENES = {
    "cornell": ("cornell_box", dict()),
    "gem": ("cornell_gem", dict()),
    "hdri": ("hdri_small", dict()),
    "cornell_hero": ("cornell_box", dict(hero_wavelengths=4)),
    "fog_medium": ("fog_ball", dict(medium_aware=True)),
}


def _hip_current_device():
    hip = C.CDLL("libamdhip64.so")   # (the process's HIP runtime, already loaded by the engine)
    dev = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(dev)) == 0
    return dev.value


def _same(got, ref, what):
    assert np.array_equal(got[1], ref[1]), what
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64)), what
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), what
    g, r = got[3], ref[3]
    assert g.kernel_launches[5] == r.kernel_launches[5], what
    assert g.camera_rays == r.camera_rays == int(ref[1].sum()), what
    assert (g.bounce_rays, g.shadow_rays, g.light_rays, g.env_hits) == (r.bounce_rays, r.shadow_rays, r.light_rays, r.env_hits), what


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GPU_SCENES))
def test_gpu_virtual_devices_equal_render_adaptive(engine, pkg, case):
    """pt_render_adaptive_multi with multi_virtual 2, 3, 4, 8 (and 4 with the RCCL exchange and gather forced) equals pt_render_adaptive bit for bit:
    film, counts, stats, rounds and the ray counters.  150 x 100 has 20 tiles with remnants; 40 x 20 has 2, so six of eight devices have no pixel."""
    scene, kw = GPU_SCENES[case]
    builder = pkg.scene.SCENES[scene]()
    a = pkg.api
    for w, h in ((150, 100), (40, 20)):
        rd = a.render_desc(w, h, 10, 5, seed=7, **kw)
        rel = pick_rel(engine, builder, rd, 0.4)
        ref = engine.create_scene(builder).render_adaptive(rd, 40, rel, step=10, stats=True)
        assert ref[1].min() < ref[1].max(), np.unique(ref[1])
        for virt, rccl in ((2, False), (3, False), (4, False), (8, False), (4, True)):
            t = engine.tuning_default()
            t.multi_virtual = virt
            if rccl:
                t.flags |= a.TUNE_MULTI_RCCL
            got = engine.create_scene(builder, t).render_adaptive_multi(rd, 40, rel, step=10, stats=True, device_mask=1)
            _same(got, ref, (case, w, virt, rccl))


@pytest.mark.gpu
def test_gpu_second_call_reuses_the_set_up_and_keeps_the_current_device(engine, pkg):
    builder = pkg.scene.cornell_box()
    a = pkg.api
    rd = a.render_desc(96, 64, 10, 5, seed=3)
    rel = pick_rel(engine, builder, rd, 0.4)
    ref = engine.create_scene(builder).render_adaptive(rd, 30, rel, stats=True)
    t = engine.tuning_default()
    t.multi_virtual = 4
    t.flags |= a.TUNE_MULTI_RCCL
    sc = engine.create_scene(builder, t)
    before = _hip_current_device()
    for call in range(2):
        got = sc.render_adaptive_multi(rd, 30, rel, stats=True, device_mask=1)
        _same(got, ref, call)
        prof = got[3]
        assert prof.seconds > 0 and prof.kernel_seconds[6] > 0
        if call == 1:
            assert prof.kernel_seconds[5] < 1e-3, prof.kernel_seconds[5]
    assert _hip_current_device() == before


@pytest.mark.gpu
def test_gpu_plain_masks_and_refusals(engine, pkg):
    """Masks 0 and 1 without virtual devices are pt_render_adaptive; a mask naming no device, a shard in the desc and null sample_counts are refused."""
    builder = pkg.scene.cornell_box()
    a = pkg.api
    rd = a.render_desc(64, 48, 10, 5, seed=5)
    rel = pick_rel(engine, builder, rd, 0.4)
    sc = engine.create_scene(builder)
    ref = sc.render_adaptive(rd, 30, rel, stats=True)
    for mask in (0, 1):
        _same(sc.render_adaptive_multi(rd, 30, rel, stats=True, device_mask=mask), ref, mask)
    with pytest.raises(a.PtError):
        sc.render_adaptive_multi(rd, 30, rel, device_mask=1 << 40)
    with pytest.raises(a.PtError):
        sc.render_adaptive_multi(a.render_desc(64, 48, 10, 5, seed=5, shard=(0, 2)), 30, rel, device_mask=1)
    film = np.zeros((48, 64, 4), np.float32)
    ad = a.AdaptiveDesc(30, 0, rel, 0.0)
    st = engine._render_adaptive_multi(sc.handle, C.byref(rd), C.byref(ad), C.c_uint64(1), film.ctypes.data_as(C.POINTER(C.c_float)), None, None, None)
    assert st == PT_ERR_INVALID_ARGUMENT and "sample_counts" in engine.last_error()
    # pt_render_adaptive keeps refusing a shard
    with pytest.raises(a.PtError) as e:
        sc.render_adaptive(a.render_desc(64, 48, 10, 5, seed=5, shard=(0, 2)), 30, rel)
    assert e.value.status == PT_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_two_physical_devices(engine, pkg):
    """The same comparison over two real devices (runs only where the box has them): the images exchanged with ncclAllReduce every round."""
    if engine.lib.pt_device_count() < 2:
        pytest.skip("one HIP device on this box")
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(150, 100, 10, 5, seed=7)
    rel = pick_rel(engine, builder, rd, 0.4)
    sc = engine.create_scene(builder)
    ref = sc.render_adaptive(rd, 40, rel, step=10, stats=True)
    for call in range(2):
        _same(sc.render_adaptive_multi(rd, 40, rel, step=10, stats=True, device_mask=0b11), ref, call)


@pytest.mark.gpu
def test_gpu_ptcli_devices(pkg, tmp_path):
    """ptcli --adaptive R --devices 1 under PT_AMD_MULTI_VIRTUAL=4 writes the films of --adaptive R alone (pt_render_adaptive_multi, and pt_render_multi
    for the setting without a sample range)."""
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    cfg = tmp_path / "config.toml"
    cfg.write_text(ADAPTIVE_CONFIG)
    runs = {"one": ([], {}), "node": (["--devices", "1"], {"PT_AMD_MULTI_VIRTUAL": "4"})}
    for name, (extra, env) in runs.items():
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / name), "--adaptive", "0.05", "--write-film"] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout + r.stderr
        assert re.search(r"adaptive: [0-9.]+ samples per pixel on average", r.stdout), r.stdout
    for f in ("adaptive.npy", "fixed.npy"):
        one, node = np.load(tmp_path / "one" / f), np.load(tmp_path / "node" / f)
        assert one.shape == node.shape and np.array_equal(one.view(np.uint32), node.view(np.uint32)), f
