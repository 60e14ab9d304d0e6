"""The spectral film on every device of a node (pt_render_spectral_multi, pt_render_adaptive_spectral_multi, include/pt_spectral.h).
Every device packs the bins of its own tiles (k_spectral_pack), hands them to the host itself and keeps them as its part of the scene's resident film; nothing is
reduced.  The CPU tier checks the pack and scatter rule the kernel compiles (csrc/pt_shard_rules.h, through tests/host_emulation/ptemu_spectral_shard.cpp)
against a numpy restatement — every pixel in exactly one shard, every bit kept —, the argument checks and the command line's refusals; the GPU tier checks the
entries with virtual devices against the one-device renders bit for bit, the node-resident film's development, repeated calls, masks and ptcli."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import emulation
from test_adaptive import pick_rel
from test_adaptive_multi import _hip_current_device
from test_spectral import scaled_c2_config
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED, PT_OK, bits, ptcli

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
u32p, f32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
F = np.float32
W, H = 77, 45   # 2 x 1 whole 32 x 32 tiles and remnant tiles on the right, at the bottom and in the corner: 6 tiles
BINS = 5


@pytest.fixture(scope="session")
def emu_sh(pkg):
    """The packed shard's rule and the node entries' argument checks on the host (ptemu_spectral_shard.cpp beside the engine's pt_plan.cpp): a library of its own."""
    L = C.CDLL(emulation.library_path("spectral_shard"))
    a = pkg.api
    L.ptemu_spectral_shard_last_error.restype = C.c_char_p
    L.ptemu_shard_pixels.restype = C.c_uint32
    L.ptemu_shard_pixels.argtypes = [C.c_uint32] * 6 + [C.c_void_p, C.c_uint32]
    L.ptemu_spectral_shard_pack.restype = None
    L.ptemu_spectral_shard_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.ptemu_spectral_shard_scatter.restype = None
    L.ptemu_spectral_shard_scatter.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    L.ptemu_spectral_multi_check.restype = C.c_int32
    L.ptemu_spectral_multi_check.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.SpectralDesc), C.c_uint32, C.c_void_p, C.c_void_p]
    L.ptemu_adaptive_spectral_multi_check.restype = C.c_int32
    L.ptemu_adaptive_spectral_multi_check.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(a.SpectralDesc), C.c_uint32, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]
    return L


# ------------------------------------------------------------------------------------------------ numpy restatement of the shard lists
def np_shard_pixels(w, h, tw, th, index, count):
    """pth::shard_pixels: the tiles in the order tests/test_adaptive_multi.py's np_owner restates (whole tiles, the right column, the bottom row, the corner),
    tile t to shard PT_TILE_SHARD = (t + t / tiles_per_row) % count (count 0: every tile); the shard's tiles taken with a stride of about 0.382 of their number,
    raised until it is coprime to it; row-major inside a tile."""
    fx, fy, rx, ry = w // tw, h // th, w % tw, h % th
    tiles = [(x * tw, x * tw + tw, y * th, y * th + th) for y in range(fy) for x in range(fx)]
    if rx:
        tiles += [(fx * tw, w, y * th, y * th + th) for y in range(fy)]
    if ry:
        tiles += [(x * tw, x * tw + tw, fy * th, h) for x in range(fx)]
        if rx:
            tiles.append((fx * tw, w, fy * th, h))
    mine = [t for t in range(len(tiles)) if count == 0 or (t + t // max(fx, 1)) % count == index]
    n = len(mine)
    stride = max(int(float(n) * 0.3819660112501051), 1)
    while math.gcd(stride, n if n else 1) != 1:
        stride += 1
    px = []
    for i in range(n):
        x0, x1, y0, y1 = tiles[mine[(i * stride) % n]]
        px += [y * w + x for y in range(y0, y1) for x in range(x0, x1)]
    return np.asarray(px, np.uint32)


def random_planes(rng, bins, n):
    """Random bit patterns, NaNs with payloads, infinities and denormals among them, with a quiet NaN of a chosen payload, a signalling-range pattern and -0.0
    put in by hand."""
    p = rng.integers(0, 2 ** 32, (bins, n), dtype=np.uint64).astype(np.uint32)
    flat = p.reshape(-1)
    flat[0] = 0x80000000                      # -0.0
    flat[-1] = 0x7FC12345                     # a quiet NaN with a payload
    flat[flat.size // 2] = 0xFF800001         # a NaN whose quiet bit is clear
    return p


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_the_node_entries_and_the_bindings_mirror_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    a = pkg.api
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pt_spectral.h")).read(), flags=re.S)

    def header_types(name):
        params = re.search(r"pt_status\s+%s\s*\((.*?)\);" % name, text, re.S).group(1)
        return [re.sub(r"\s+", " ", p.strip().rsplit(" ", 1)[0].replace("*", " *")).replace(" *", "*") for p in params.split(",")]
    L = a.Library(pkg.LIBRARY_PATH)
    cases = {
        "render_spectral_multi": (["pt_scene*", "const pt_render_desc*", "const pt_spectral_desc*", "uint64_t", "float*", "float*", "pt_profile*"],
                                  [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.SpectralDesc), C.c_uint64, f32p, f32p, C.POINTER(a.Profile)]),
        "render_adaptive_spectral_multi": (["pt_scene*", "const pt_render_desc*", "const pt_adaptive_desc*", "const pt_spectral_desc*", "uint64_t", "float*", "uint32_t*",
                                            "double*", "float*", "pt_profile*"],
                                           [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(a.SpectralDesc), C.c_uint64, f32p, u32p, f64p, f32p,
                                            C.POINTER(a.Profile)]),
    }
    for name, (types, want) in cases.items():
        assert hasattr(lib, "pt_" + name), name
        assert name not in a.API_FUNCTIONS   # (pt_spectral.h, not the oracle's boundary)
        assert header_types("pt_" + name) == types, name
        fn = getattr(L, "_" + name)
        assert fn is not None and list(fn.argtypes) == want and fn.restype == C.c_int32, name
    # the Python methods: the one-device ones' parameters, then the mask
    for single, multi in ((a.Scene.render_spectral, a.Scene.render_spectral_multi), (a.Scene.render_adaptive_spectral, a.Scene.render_adaptive_spectral_multi)):
        assert list(inspect.signature(multi).parameters) == list(inspect.signature(single).parameters) + ["device_mask"]
        assert inspect.signature(multi).parameters["device_mask"].default == 0
    den = inspect.signature(a.Scene.render_denoised_spectral).parameters
    assert list(den)[-1] == "device_mask" and den["device_mask"].default is None


FILMS = [(77, 45), (40, 20), (32, 32), (1, 1)]


@pytest.mark.parametrize("w,h", FILMS)
def test_pack_and_scatter_keep_every_bit_and_write_every_pixel_once(emu_sh, w, h):
    """For N = 1, 2, 3, 4, 8 shards and B = 1, 5, 64 bins over planes of random bit patterns: the shard lists are the numpy restatement's and partition the film
    (every pixel in exactly one list); each shard's packed planes are planes[:, px]; scattering every shard into planes filled with a marker returns the input,
    compared as u32.  With 8 shards of a 40 x 20 film (2 tiles) six shards are empty."""
    npx = w * h
    for n in (1, 2, 3, 4, 8):
        lists = []
        for v in range(n):
            index, count = (v, n) if n > 1 else (0, 0)   # (one device: the engine leaves the desc without shards)
            px = np.zeros(npx, np.uint32)
            k = emu_sh.ptemu_shard_pixels(w, h, 32, 32, index, count, px.ctypes.data, npx)
            want = np_shard_pixels(w, h, 32, 32, index, count)
            assert k == want.size and np.array_equal(px[:k], want), (n, v)
            lists.append(px[:k].copy())
        written = np.zeros(npx, np.int64)
        for px in lists:
            np.add.at(written, px, 1)
        assert np.array_equal(written, np.ones(npx, np.int64)), n                      # every pixel in exactly one shard
        if (w, h, n) == (40, 20, 8):
            assert sorted(len(px) for px in lists) == [0] * 6 + [8 * 20, 32 * 20]
        for B in (1, 5, 64):
            rng = np.random.default_rng(100000 * w + 1000 * n + B)
            planes = random_planes(rng, B, npx)
            back = np.full((B, npx), 0xDEADBEEF, np.uint32)
            stores = np.zeros((B, npx), np.int64)
            for px in lists:
                k = px.size
                packed = np.full((B, max(k, 1)), 0xABABABAB, np.uint32)
                if k:                                                                     # (an empty shard launches nothing and copies nothing)
                    emu_sh.ptemu_spectral_shard_pack(planes.ctypes.data, npx, px.ctypes.data, k, B, packed.ctypes.data)
                    assert np.array_equal(packed[:, :k], planes[:, px]), (n, B)
                    emu_sh.ptemu_spectral_shard_scatter(packed.ctypes.data, px.ctypes.data, k, B, back.ctypes.data, npx)
                    stores[:, px] += 1
            assert np.array_equal(back, planes), (n, B)
            assert np.array_equal(stores, np.ones((B, npx), np.int64)), (n, B)
            if npx > 2:   # (the hand-made patterns are among what came back)
                assert back.reshape(-1)[0] == 0x80000000 and back.reshape(-1)[-1] == 0x7FC12345 and back.reshape(-1)[back.size // 2] == 0xFF800001


def test_the_node_entries_refuse_each_bad_argument_with_its_own_message(emu_sh, pkg):
    """check_spectral_multi_args and check_adaptive_spectral_args through the emulation, without a device, then the product's entries, which run them before they
    look for one."""
    a = pkg.api
    msgs = {}
    film, spectral, counts = np.zeros((8, 8, 4), F), np.zeros((5, 8, 8), F), np.zeros((8, 8), np.uint32)
    scene = C.c_void_p(1)   # (only compared with null)

    def sdesc(bins=5, reserved=0):
        sd = a.SpectralDesc(bins)
        sd.reserved[1] = reserved
        return sd

    def fixed(key, rd=None, sd=None, f=film, s=spectral, sc=scene):
        rd = rd or a.render_desc(8, 8, 10, 3)
        sd = sd or sdesc()
        st = emu_sh.ptemu_spectral_multi_check(sc, C.byref(rd), C.byref(sd), 1, f.ctypes.data if f is not None else None, s.ctypes.data if s is not None else None)
        if st != PT_OK:
            msgs.setdefault(key, set()).add((st, emu_sh.ptemu_spectral_shard_last_error().decode()))
        return st

    def adaptive(key, rd=None, sd=None, f=film, s=spectral, c=counts, mx=30):
        rd = rd or a.render_desc(8, 8, 10, 3)
        sd = sd or sdesc()
        ad = a.AdaptiveDesc(mx, 10, 0.1, 0.0)
        st = emu_sh.ptemu_adaptive_spectral_multi_check(scene, C.byref(rd), C.byref(ad), C.byref(sd), 1, f.ctypes.data if f is not None else None,
                                                        c.ctypes.data if c is not None else None, s.ctypes.data if s is not None else None)
        if st != PT_OK:
            msgs.setdefault(key, set()).add((st, emu_sh.ptemu_spectral_shard_last_error().decode()))
        return st

    assert fixed("ok") == PT_OK and adaptive("ok") == PT_OK and "ok" not in msgs
    assert fixed("ok", rd=a.render_desc(8, 8, 20, 3, first_sample=10, sample_count=10)) == PT_OK        # (a partial range is pt_render_spectral's)
    for check in (fixed, adaptive):
        name = check.__name__
        assert check(name + "_b0", sd=sdesc(0)) == PT_ERR_INVALID_ARGUMENT and check(name + "_b65", sd=sdesc(65)) == PT_ERR_INVALID_ARGUMENT
        assert check(name + "_reserved", sd=sdesc(5, 1)) == PT_ERR_INVALID_ARGUMENT
        assert check(name + "_film", f=None) == PT_ERR_INVALID_ARGUMENT and check(name + "_spectral", s=None) == PT_ERR_INVALID_ARGUMENT
    assert adaptive("adaptive_counts", c=None) == PT_ERR_INVALID_ARGUMENT
    assert fixed("fixed_shard", rd=a.render_desc(8, 8, 10, 3, shard=(0, 2))) == PT_ERR_INVALID_ARGUMENT
    assert fixed("fixed_shard", rd=a.render_desc(8, 8, 10, 3, shard=(0, 1))) == PT_ERR_INVALID_ARGUMENT  # (shard_count must be 0, not "at most one shard")
    assert adaptive("adaptive_shard", rd=a.render_desc(8, 8, 10, 3, shard=(0, 2))) == PT_ERR_UNSUPPORTED
    assert fixed("fixed_scene", sc=None) == PT_ERR_INVALID_ARGUMENT
    assert fixed("fixed_size", rd=a.render_desc(0, 8, 10, 3)) == PT_ERR_INVALID_ARGUMENT
    assert fixed("fixed_camera", rd=a.render_desc(8, 8, 10, 3, camera_index=1)) == PT_ERR_INVALID_ARGUMENT
    assert all(len(v) == 1 for v in msgs.values()), msgs
    flat = {k: next(iter(v))[1] for k, v in msgs.items()}
    for key in ("b0", "b65", "reserved", "film", "spectral"):                           # the same rule, the same words in both entries
        assert flat["fixed_" + key] == flat["adaptive_" + key], key
    own = [flat["fixed_" + k] for k in ("b0", "b65", "reserved", "film", "spectral", "shard", "scene", "size", "camera")] + [flat["adaptive_counts"], flat["adaptive_shard"]]
    assert len(set(own)) == len(own), flat
    assert "64" in flat["fixed_b65"] and "reserved" in flat["fixed_reserved"] and "film_xyzw" in flat["fixed_film"] and "spectral" in flat["fixed_spectral"]
    assert "shard_count must be 0" in flat["fixed_shard"] and "shard_count 0" in flat["adaptive_shard"] and "sample_counts" in flat["adaptive_counts"]
    # the product runs the same checks before it looks for a device: without one (and so without a scene) the first of them is the one that can be seen
    L = pkg.load()
    rd, sd, ad = a.render_desc(8, 8, 10, 3), a.SpectralDesc(5), a.AdaptiveDesc(30, 10, 0.1, 0.0)
    assert L._render_spectral_multi(None, C.byref(rd), C.byref(sd), 0, film.ctypes.data_as(f32p), spectral.ctypes.data_as(f32p), None) == PT_ERR_INVALID_ARGUMENT
    assert L.last_error() == flat["fixed_scene"]
    assert L._render_adaptive_spectral_multi(None, C.byref(rd), C.byref(ad), C.byref(sd), 0, film.ctypes.data_as(f32p), counts.ctypes.data_as(u32p), None,
                                             spectral.ctypes.data_as(f32p), None) == PT_ERR_INVALID_ARGUMENT
    assert L.last_error() == flat["fixed_scene"]


def test_ptcli_refuses_bad_spectral_devices_while_parsing(pkg, tmp_path):
    """Each refusal exits with status 2 and its own message before any file is read; the refusals of --devices with the spectral flags stay what they were."""
    exe = ptcli(pkg)
    cases = [
        (["--spectral-devices", "1"], "--spectral-devices needs --spectral-bins or --denoise-spectral-bins"),
        (["--denoise", "--spectral-devices", "1"], "--spectral-devices needs --spectral-bins or --denoise-spectral-bins"),
        (["--spectral-bins", "8", "--spectral-devices", "1", "--devices", "1"], "--spectral-devices cannot be combined with --devices"),
        (["--denoise", "--denoise-spectral-bins", "8", "--devices", "1", "--spectral-devices", "1"], "--spectral-devices cannot be combined with --devices"),
        (["--spectral-bins", "8", "--spectral-devices", "x"], "--spectral-devices needs a device mask"),
        (["--spectral-bins", "8", "--spectral-devices", "3q"], "--spectral-devices needs a device mask"),
        (["--spectral-bins", "8", "--spectral-devices"], "--spectral-devices needs a value"),
        (["--spectral-bins", "8", "--devices", "6"], "--spectral-bins cannot be combined with --devices naming more than one GPU: pt_render_multi has no spectral film"),
        (["--spectral-bins", "8", "--devices", "2"], "--spectral-bins renders on device 0: --devices may name that device alone"),
        (["--denoise", "--denoise-spectral-bins", "8", "--devices", "3"], "--denoise-spectral-bins renders on device 0: --devices may name that device alone"),
    ]
    seen = set()
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
        seen.add(message)
    assert len(seen) == 7
    assert "--spectral-devices MASK" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    head = open(os.path.join(CSRC, "host", "ptcli.cpp")).read().split("#include")[0]
    assert "[--spectral-devices MASK]" in head
    # a dry run with the flag parses and ends well
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    ok = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n", "--spectral-bins", "8", "--spectral-devices", "0x1"],
                        capture_output=True, text=True, cwd=str(tmp_path))
    assert ok.returncode == 0, ok.stderr


# ------------------------------------------------------------------------------------------------ GPU tier
GPU_SCENES = {
    "cornell": ("cornell_box", dict()),
    "cornell_hero": ("cornell_box", dict(hero_wavelengths=4)),
    "gem": ("cornell_gem", dict()),
}
COUNTERS = ("camera_rays", "bounce_rays", "shadow_rays", "light_rays", "env_hits")


def tuned_scene(engine, pkg, builder, virt=0, rccl=False):
    t = engine.tuning_default()
    t.multi_virtual = virt
    if rccl:
        t.flags |= pkg.api.TUNE_MULTI_RCCL
    return engine.create_scene(builder, t)


def same_fixed(got, ref, what):
    assert np.array_equal(bits(got[0]), bits(ref[0])), what
    assert np.array_equal(bits(got[1]), bits(ref[1])), what
    assert [getattr(got[2], c) for c in COUNTERS] == [getattr(ref[2], c) for c in COUNTERS], what


def same_adaptive(got, ref, what):
    """(film, counts, stats, spectral, profile)"""
    assert np.array_equal(got[1], ref[1]), what
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64)), what
    assert np.array_equal(bits(got[0]), bits(ref[0])), what
    assert np.array_equal(bits(got[3]), bits(ref[3])), what
    g, r = got[4], ref[4]
    assert g.kernel_launches[5] == r.kernel_launches[5], what
    assert g.camera_rays == r.camera_rays == int(ref[1].sum()), what
    assert [getattr(g, c) for c in COUNTERS] == [getattr(r, c) for c in COUNTERS], what


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GPU_SCENES))
def test_gpu_virtual_devices_equal_render_spectral(engine, pkg, case):
    """pt_render_spectral_multi on a 77 x 45 film, 20 spp, 5 bins, with multi_virtual 2, 3, 4, 4 with the RCCL path forced, and the RCCL path alone (one shard
    that is the whole film): film and bins as u32 and the five ray counters are pt_render_spectral's."""
    scene, kw = GPU_SCENES[case]
    builder = pkg.scene.SCENES[scene]()
    rd = pkg.api.render_desc(W, H, 20, 4, seed=7, **kw)
    ref = engine.create_scene(builder).render_spectral(rd, BINS)
    assert np.any(ref[1] != 0)
    for virt, rccl in ((2, False), (3, False), (4, False), (4, True), (0, True)):
        got = tuned_scene(engine, pkg, builder, virt, rccl).render_spectral_multi(rd, BINS, device_mask=1)
        same_fixed(got, ref, (case, virt, rccl))


@pytest.mark.gpu
def test_gpu_empty_shards_many_bins_and_a_partial_range(engine, pkg):
    """40 x 20 with multi_virtual 8: two tiles, six devices without a pixel.  64 bins on the 77 x 45 film.  Samples 10..19 of 20: the running sums of
    pt_render_spectral for the same desc."""
    a = pkg.api
    builder = pkg.scene.cornell_box()
    one = engine.create_scene(builder)
    rd = a.render_desc(40, 20, 20, 4, seed=7)
    same_fixed(tuned_scene(engine, pkg, builder, 8).render_spectral_multi(rd, BINS, device_mask=1), one.render_spectral(rd, BINS), "8 devices, 2 tiles")
    node = tuned_scene(engine, pkg, builder, 3)
    rd = a.render_desc(W, H, 20, 4, seed=7)
    same_fixed(node.render_spectral_multi(rd, 64, device_mask=1), one.render_spectral(rd, 64), "64 bins")
    part = a.render_desc(W, H, 20, 4, seed=7, first_sample=10, sample_count=10)
    ref = one.render_spectral(part, BINS)
    whole = one.render_spectral(rd, BINS)
    assert not np.array_equal(bits(ref[1]), bits(whole[1]))
    same_fixed(node.render_spectral_multi(part, BINS, device_mask=1), ref, "partial range")


@pytest.mark.gpu
def test_gpu_virtual_devices_equal_render_adaptive_spectral(engine, pkg):
    """pt_render_adaptive_spectral_multi, 77 x 45, 10 to 40 spp in steps of 10 with counts that differ between pixels, multi_virtual 2, 3, 8 and 4 with RCCL forced:
    film, counts, stats, bins, rounds and the ray counters are pt_render_adaptive_spectral's."""
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(W, H, 10, 4, seed=7)
    rel = pick_rel(engine, builder, rd, 0.4)
    ref = engine.create_scene(builder).render_adaptive_spectral(rd, BINS, 40, rel, step=10, stats=True)
    assert ref[1].min() < ref[1].max(), np.unique(ref[1])
    assert ref[4].kernel_launches[5] > 1
    for virt, rccl in ((2, False), (3, False), (8, False), (4, True)):
        got = tuned_scene(engine, pkg, builder, virt, rccl).render_adaptive_spectral_multi(rd, BINS, 40, rel, step=10, stats=True, device_mask=1)
        same_adaptive(got, ref, (virt, rccl))


@pytest.mark.gpu
def test_gpu_node_resident_film(engine, pkg):
    """After a node render the resident film is the packed shards: pt_spectral_resident tells its size, pt_spectral_project_resident (K = 3: one launch per shard;
    K = 11: two) is pt_spectral_project of the returned array bit for bit, for the fixed and the adaptive entry; a later one-device render replaces it, and a node
    call that is refused leaves the scene without one."""
    a = pkg.api
    builder = pkg.scene.cornell_box()
    sc = tuned_scene(engine, pkg, builder, 3)
    rng = np.random.default_rng(11)
    rd = a.render_desc(W, H, 20, 4, seed=7)
    assert sc.spectral_resident() is None
    _, S, _ = sc.render_spectral_multi(rd, BINS, device_mask=1)
    assert sc.spectral_resident() == (W, H, BINS)
    for K in (3, 11):
        M = rng.uniform(-2.0, 2.0, (K, BINS)).astype(F)
        got = sc.spectral_project_resident(M)
        assert got.shape == (K, H, W) and np.any(got != 0)
        assert np.array_equal(bits(got), bits(engine.spectral_project(S, M))), K
    # the adaptive entry, another number of bins
    rda = a.render_desc(W, H, 10, 4, seed=7)
    _, counts, Sa, _ = sc.render_adaptive_spectral_multi(rda, 7, 30, 0.05, device_mask=1)
    assert sc.spectral_resident() == (W, H, 7)
    M = rng.uniform(-2.0, 2.0, (11, 7)).astype(F)
    assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(engine.spectral_project(Sa, M)))
    # a one-device render at another size replaces the resident film
    rd2 = a.render_desc(16, 8, 4, 4, seed=4)
    _, S2, _ = sc.render_spectral(rd2, 6)
    assert sc.spectral_resident() == (16, 8, 6)
    M = rng.uniform(-2.0, 2.0, (3, 6)).astype(F)
    assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(engine.spectral_project(S2, M)))
    # and a node render after it is resident again
    _, S, _ = sc.render_spectral_multi(rd, BINS, device_mask=1)
    M = rng.uniform(-2.0, 2.0, (3, BINS)).astype(F)
    assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(engine.spectral_project(S, M)))
    # a node call that fails in its checks: no resident film afterwards
    for refused in (lambda: sc.render_spectral_multi(a.render_desc(W, H, 20, 4, seed=7, shard=(0, 2)), BINS, device_mask=1),
                    lambda: sc.render_spectral_multi(rd, BINS, device_mask=1 << 40),
                    lambda: sc.render_adaptive_spectral_multi(a.render_desc(W, H, 15, 4, seed=7), BINS, 30, 0.05, device_mask=1)):
        sc.render_spectral_multi(rd, BINS, device_mask=1)
        assert sc.spectral_resident() == (W, H, BINS)
        with pytest.raises(a.PtError):
            refused()
        assert sc.spectral_resident() is None
        with pytest.raises(a.PtError, match="no resident spectral film"):
            sc.spectral_project_resident(M)


@pytest.mark.gpu
def test_gpu_second_call_reuses_the_set_up_and_keeps_the_current_device(engine, pkg):
    a = pkg.api
    builder = pkg.scene.cornell_box()
    rd = a.render_desc(W, H, 10, 4, seed=3)
    one = engine.create_scene(builder)
    ref = one.render_spectral(rd, BINS)
    rel = pick_rel(engine, builder, rd, 0.4)
    ref_a = one.render_adaptive_spectral(rd, BINS, 30, rel, stats=True)
    sc = tuned_scene(engine, pkg, builder, 4, rccl=True)
    before = _hip_current_device()
    for call in range(2):
        got = sc.render_spectral_multi(rd, BINS, device_mask=1)
        same_fixed(got, ref, call)
        prof = got[2]
        assert prof.seconds > 0 and prof.kernel_seconds[6] > 0
        if call == 1:
            assert prof.kernel_seconds[5] < 1e-3, prof.kernel_seconds[5]
    for call in range(2):
        got = sc.render_adaptive_spectral_multi(rd, BINS, 30, rel, stats=True, device_mask=1)
        same_adaptive(got, ref_a, call)
        prof = got[4]
        assert prof.seconds > 0 and prof.kernel_seconds[6] > 0
        if call == 1:
            assert prof.kernel_seconds[5] < 1e-3, prof.kernel_seconds[5]
    sc.spectral_project_resident(np.ones((3, BINS), F))
    assert _hip_current_device() == before


@pytest.mark.gpu
def test_gpu_plain_masks_and_refusals(engine, pkg):
    """Masks 0 and 1 without virtual devices are the one-device renders (on a box with one GPU, mask 0 too); a mask naming no device is refused."""
    a = pkg.api
    builder = pkg.scene.cornell_box()
    rd = a.render_desc(64, 48, 10, 4, seed=5)
    sc = engine.create_scene(builder)
    ref = sc.render_spectral(rd, BINS)
    rel = pick_rel(engine, builder, rd, 0.4)
    ref_a = sc.render_adaptive_spectral(rd, BINS, 30, rel, stats=True)
    for mask in (0, 1):
        same_fixed(sc.render_spectral_multi(rd, BINS, device_mask=mask), ref, mask)
        same_adaptive(sc.render_adaptive_spectral_multi(rd, BINS, 30, rel, stats=True, device_mask=mask), ref_a, mask)
    with pytest.raises(a.PtError, match="names no visible HIP device"):
        sc.render_spectral_multi(rd, BINS, device_mask=1 << 40)
    with pytest.raises(a.PtError, match="names no visible HIP device"):
        sc.render_adaptive_spectral_multi(rd, BINS, 30, rel, device_mask=1 << 40)
    with pytest.raises(a.PtError, match="shard_count must be 0"):
        sc.render_spectral_multi(a.render_desc(64, 48, 10, 4, seed=5, shard=(0, 2)), BINS, device_mask=1)
    # render_denoised_spectral through the node call: the one-device outputs
    node = tuned_scene(engine, pkg, builder, 2)
    rdd = a.render_desc(32, 32, 20, 4, seed=5)
    want = sc.render_denoised_spectral(rdd, BINS)
    got = node.render_denoised_spectral(rdd, BINS, device_mask=1)
    for g, w_ in zip(got[:4], want[:4]):
        assert np.array_equal(bits(g), bits(w_))
    assert np.array_equal(got[4], want[4])


@pytest.mark.gpu
def test_gpu_two_physical_devices(engine, pkg):
    """The same comparisons over two real devices (runs only where the box has them)."""
    if engine.lib.pt_device_count() < 2:
        pytest.skip("one HIP device on this box")
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(W, H, 10, 4, seed=7)
    rel = pick_rel(engine, builder, rd, 0.4)
    sc = engine.create_scene(builder)
    ref = sc.render_spectral(rd, BINS)
    ref_a = sc.render_adaptive_spectral(rd, BINS, 40, rel, step=10, stats=True)
    for call in range(2):
        got = sc.render_spectral_multi(rd, BINS, device_mask=0b11)
        same_fixed(got, ref, call)
        M = np.random.default_rng(call).uniform(-2.0, 2.0, (11, BINS)).astype(F)
        assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(engine.spectral_project(got[1], M)))
        same_adaptive(sc.render_adaptive_spectral_multi(rd, BINS, 40, rel, step=10, stats=True, device_mask=0b11), ref_a, call)


PTCLI_RUNS = {
    "spectral_bins": (["--spectral-bins", "8", "--develop", "cie"],
                      ["beauty.exr", "beauty.png", "beauty_developed.exr", "beauty_developed.png", "beauty_spectral.exr"]),
    "denoise_spectral_bins": (["--denoise", "--denoise-spectral-bins", "8"],
                              ["beauty.exr", "beauty.png", "beauty_denoised.exr", "beauty_denoised.png", "beauty_denoised_spectral.exr", "beauty_spectral.exr"]),
    "denoise_spectral_bins_develop": (["--denoise", "--denoise-spectral-bins", "8", "--develop", "cie"],
                                      ["beauty.exr", "beauty.png", "beauty_denoised.exr", "beauty_denoised.png", "beauty_denoised_developed.exr", "beauty_denoised_developed.png",
                                       "beauty_denoised_spectral.exr", "beauty_developed.exr", "beauty_developed.png", "beauty_spectral.exr"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(PTCLI_RUNS))
def test_gpu_ptcli_spectral_devices(pkg, tmp_path, mode):
    """ptcli with --spectral-devices 1 under PT_AMD_MULTI_VIRTUAL=4 (the node calls, four shards; --develop through the node-resident film) writes every file of
    the run without the flag, byte for byte."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    args, files = PTCLI_RUNS[mode]
    runs = {"one": ([], {}), "node": (["--spectral-devices", "1"], {"PT_AMD_MULTI_VIRTUAL": "4"})}
    for name, (extra, env) in runs.items():
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / name)] + args + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(str(tmp_path / name))) == files
    for f in files:
        assert (tmp_path / "one" / f).read_bytes() == (tmp_path / "node" / f).read_bytes(), f
