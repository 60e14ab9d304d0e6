"""Light groups on every device of a node (pt_render_light_groups_multi, pt_render_adaptive_light_groups_multi, include/pt_light_groups_multi.h, DESIGN.md section
15 "On every device of a node").  Every device packs the group films of its own tiles (k_light_groups_pack), hands them to the host itself and keeps them as its
part of the scene's resident group films; nothing is reduced.  The CPU tier checks the pack, scatter and unpack rule the kernels compile
(csrc/pt_shard_rules.h, through tests/host_emulation/ptemu_light_groups_shard.cpp) — every pixel in exactly one shard, every bit kept —, the argument
checks, the command line's refusals and the sanitizer program; the GPU tier checks the entries with virtual devices against the one-device renders bit for bit, the
node-resident mix, the assemble for the filter, repeated calls, masks and ptcli."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import emulation
from test_adaptive import pick_rel
from test_adaptive_multi import _hip_current_device
from test_light_groups import ROOM_ENV_GROUP, ROOM_GROUPS, clean_tuning, emissive_mesh_scene, scaled_c2_config
from test_spectral_multi import np_shard_pixels
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED, PT_OK, bits, ptcli

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "pt_light_groups_multi.h")
u32p, f32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
F = np.float32
W, H = 77, 45   # 2 x 1 whole 32 x 32 tiles and remnant tiles on the right, at the bottom and in the corner: 6 tiles
COUNTERS = ("camera_rays", "bounce_rays", "shadow_rays", "light_rays", "env_hits")


@pytest.fixture(scope="session")
def emu_gs(pkg):
    """The packed group shard's rule and the node entries' argument checks on the host (ptemu_light_groups_shard.cpp beside the engine's pt_plan.cpp)."""
    L = C.CDLL(emulation.library_path("light_groups_shard"))
    a = pkg.api
    L.ptemu_light_groups_shard_last_error.restype = C.c_char_p
    L.ptemu_lg_shard_pixels.restype = C.c_uint32
    L.ptemu_lg_shard_pixels.argtypes = [C.c_uint32] * 6 + [C.c_void_p, C.c_uint32]
    L.ptemu_light_groups_shard_pack.restype = None
    L.ptemu_light_groups_shard_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    for name in ("ptemu_light_groups_shard_scatter", "ptemu_light_groups_shard_unpack"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    L.ptemu_light_groups_multi_check.restype = C.c_int32
    L.ptemu_light_groups_multi_check.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.LightGroupsDesc), C.c_uint32, C.c_uint32, C.c_void_p]
    L.ptemu_adaptive_light_groups_multi_check.restype = C.c_int32
    L.ptemu_adaptive_light_groups_multi_check.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(a.LightGroupsDesc), C.c_uint32, C.c_uint32,
                                                          C.c_void_p, C.c_void_p]
    L.ptemu_light_groups_one_check.restype = C.c_int32
    L.ptemu_light_groups_one_check.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.LightGroupsDesc), C.c_uint32, C.c_void_p]
    return L


def random_films(rng, G, n):
    """Random bit patterns, NaNs with payloads, infinities and denormals among them, with -0.0, a quiet NaN of a chosen payload and a NaN whose quiet bit is
    clear put in by hand: [G, n, 4] as u32."""
    p = rng.integers(0, 2 ** 32, (G, n, 4), dtype=np.uint64).astype(np.uint32)
    flat = p.reshape(-1)
    flat[0] = 0x80000000
    flat[-1] = 0x7FC12345
    flat[flat.size // 2] = 0xFF800001
    return p


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_the_node_entries_and_the_bindings_mirror_the_header(pkg, tmp_path):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    a = pkg.api
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def header_types(name):
        params = re.search(r"pt_status\s+%s\s*\((.*?)\);" % name, text, re.S).group(1)
        return [re.sub(r"\s+", " ", p.strip().rsplit(" ", 1)[0].replace("*", " *")).replace(" *", "*") for p in params.split(",")]
    L = a.Library(pkg.LIBRARY_PATH)
    cases = {
        "render_light_groups_multi": (["pt_scene*", "const pt_render_desc*", "const pt_light_groups_desc*", "uint64_t", "float*", "float*", "pt_profile*"],
                                      [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.LightGroupsDesc), C.c_uint64, f32p, f32p, C.POINTER(a.Profile)]),
        "render_adaptive_light_groups_multi": (["pt_scene*", "const pt_render_desc*", "const pt_adaptive_desc*", "const pt_light_groups_desc*", "uint64_t", "float*",
                                                "uint32_t*", "double*", "float*", "pt_profile*"],
                                               [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.AdaptiveDesc), C.POINTER(a.LightGroupsDesc), C.c_uint64, f32p, u32p, f64p,
                                                f32p, C.POINTER(a.Profile)]),
    }
    for name, (types, want) in cases.items():
        assert hasattr(lib, "pt_" + name), name
        assert name not in a.API_FUNCTIONS   # (pt_light_groups_multi.h, not the oracle's boundary)
        assert header_types("pt_" + name) == types, name
        fn = getattr(L, "_" + name)
        assert fn is not None and list(fn.argtypes) == want and fn.restype == C.c_int32, name
    # the Python methods: the one-device ones' parameters, then the mask
    for single, multi in ((a.Scene.render_light_groups, a.Scene.render_light_groups_multi), (a.Scene.render_adaptive_light_groups, a.Scene.render_adaptive_light_groups_multi)):
        assert list(inspect.signature(multi).parameters) == list(inspect.signature(single).parameters) + ["device_mask"]
        assert inspect.signature(multi).parameters["device_mask"].default == 0
    den = inspect.signature(a.Scene.render_denoised_light_groups).parameters
    assert list(den)[-2:] == ["device_mask", "assemble"] and den["device_mask"].default is None and den["assemble"].default is False
    # the header compiles alone, as C
    src = tmp_path / "alone.c"
    src.write_text('#include "pt_light_groups_multi.h"\nint main(void) { return PT_LIGHT_GROUPS_MAX == 8 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "alone.o")])


FILMS = [(77, 45), (40, 20), (32, 32), (1, 1)]


@pytest.mark.parametrize("w,h", FILMS)
def test_pack_scatter_and_unpack_keep_every_bit_and_write_every_pixel_once(emu_gs, w, h):
    """For N = 1, 2, 3, 4, 8 shards and G = 1, 3, 8 groups over group films of random bit patterns: the shard lists are the numpy restatement's and partition the
    film (every pixel in exactly one list); each shard's packed films are films[:, px]; scattering every shard (the host threads' rule) and unpacking every shard
    (k_light_groups_unpack's rule) into films filled with a marker both return the input, compared as u32.  With 8 shards of a 40 x 20 film (2 tiles) six shards
    are empty."""
    npx = w * h
    for n in (1, 2, 3, 4, 8):
        lists = []
        for v in range(n):
            index, count = (v, n) if n > 1 else (0, 0)   # (one device: the engine leaves the desc without shards)
            px = np.zeros(npx, np.uint32)
            k = emu_gs.ptemu_lg_shard_pixels(w, h, 32, 32, index, count, px.ctypes.data, npx)
            want = np_shard_pixels(w, h, 32, 32, index, count)
            assert k == want.size and np.array_equal(px[:k], want), (n, v)
            lists.append(px[:k].copy())
        written = np.zeros(npx, np.int64)
        for px in lists:
            np.add.at(written, px, 1)
        assert np.array_equal(written, np.ones(npx, np.int64)), n                      # every pixel in exactly one shard
        if (w, h, n) == (40, 20, 8):
            assert sorted(len(px) for px in lists) == [0] * 6 + [8 * 20, 32 * 20]
        for G in (1, 3, 8):
            rng = np.random.default_rng(100000 * w + 1000 * n + G)
            films = random_films(rng, G, npx)
            scattered = np.full((G, npx, 4), 0xDEADBEEF, np.uint32)
            unpacked = np.full((G, npx, 4), 0xDEADBEEF, np.uint32)
            stores = np.zeros((G, npx), np.int64)
            for px in lists:
                k = px.size
                if k == 0:                                                                # (an empty shard launches nothing and copies nothing)
                    continue
                packed = np.full((G, k, 4), 0xABABABAB, np.uint32)
                emu_gs.ptemu_light_groups_shard_pack(films.ctypes.data, npx, px.ctypes.data, k, G, packed.ctypes.data)
                assert np.array_equal(packed, films[:, px]), (n, G)
                emu_gs.ptemu_light_groups_shard_scatter(packed.ctypes.data, px.ctypes.data, k, G, scattered.ctypes.data, npx)
                emu_gs.ptemu_light_groups_shard_unpack(packed.ctypes.data, px.ctypes.data, k, G, unpacked.ctypes.data, npx)
                stores[:, px] += 1
            assert np.array_equal(scattered, films), (n, G)
            assert np.array_equal(unpacked, films), (n, G)
            assert np.array_equal(stores, np.ones((G, npx), np.int64)), (n, G)
            for back in (scattered, unpacked):   # (the hand-made patterns are among what came back)
                flat = back.reshape(-1)
                assert flat[0] == 0x80000000 and flat[-1] == 0x7FC12345 and flat[flat.size // 2] == 0xFF800001


def test_the_node_entries_refuse_each_bad_argument_with_its_own_message(emu_gs, pkg):
    """check_light_groups_multi_args and check_adaptive_light_groups_multi_args through the emulation, without a device: everything the one-device check refuses,
    with its words, except the shard, which is the node entries' own refusal; then the product's entries, which run the same checks before they look for a device."""
    a = pkg.api
    msgs = {}
    film, counts = np.zeros((8, 8, 4), F), np.zeros((8, 8), np.uint32)
    scene = C.c_void_p(1)   # (only compared with null)
    ids = np.array([0, 1, 2, 0, 1, 2], np.uint8)

    def gdesc(G=3, n=6, env=0, table=ids, reserved=0):
        gd = a.LightGroupsDesc(G, n, table.ctypes.data_as(C.POINTER(C.c_uint8)) if table is not None else None, env)
        gd.reserved[1] = reserved
        return gd

    def note(key, st):
        if st != PT_OK:
            msgs.setdefault(key, set()).add((st, emu_gs.ptemu_light_groups_shard_last_error().decode()))
        return st

    def fixed(key, rd=None, gd=None, f=film, sc=scene, instances=6, null_rd=False, null_gd=False):
        rd = rd or a.render_desc(8, 8, 10, 3)
        gd = gd or gdesc()
        return note(key, emu_gs.ptemu_light_groups_multi_check(sc, None if null_rd else C.byref(rd), None if null_gd else C.byref(gd), instances, 1,
                                                               f.ctypes.data if f is not None else None))

    def adaptive(key, rd=None, gd=None, f=film, sc=scene, instances=6, null_rd=False, null_gd=False, c=counts, ad=None, null_ad=False):
        rd = rd or a.render_desc(8, 8, 10, 3)
        gd = gd or gdesc()
        ad = ad or a.AdaptiveDesc(30, 10, 0.1, 0.0)
        return note(key, emu_gs.ptemu_adaptive_light_groups_multi_check(sc, None if null_rd else C.byref(rd), None if null_ad else C.byref(ad),
                                                                        None if null_gd else C.byref(gd), instances, 1, f.ctypes.data if f is not None else None,
                                                                        c.ctypes.data if c is not None else None))

    def one(rd=None, gd=None):
        rd = rd or a.render_desc(8, 8, 10, 3)
        gd = gd or gdesc()
        st = emu_gs.ptemu_light_groups_one_check(scene, C.byref(rd), C.byref(gd), 6, film.ctypes.data)
        return st, emu_gs.ptemu_light_groups_shard_last_error().decode()

    assert fixed("ok") == PT_OK and adaptive("ok") == PT_OK and "ok" not in msgs
    INV, UNS = PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED
    shared = {   # key: (keyword arguments, status, a word of the message)
        "scene": (dict(sc=None), INV, "scene is null"), "rd": (dict(null_rd=True), INV, "render desc is null"), "gd": (dict(null_gd=True), INV, "light groups desc is null"),
        "film": (dict(f=None), INV, "film_xyzw is null"), "g0": (dict(gd=gdesc(G=0)), INV, "group_count must be in 1..8"), "g9": (dict(gd=gdesc(G=9)), INV, "group_count must be in 1..8"),
        "reserved": (dict(gd=gdesc(reserved=1)), INV, "reserved must be 0"), "id": (dict(gd=gdesc(G=2)), INV, "group ids must be below group_count"),
        "count": (dict(instances=7), INV, "the scene has 7 instances"), "table": (dict(gd=gdesc(table=None)), INV, "instance_group is null"),
        "env": (dict(gd=gdesc(env=3)), INV, "environment_group must be below group_count"),
        "hero": (dict(rd=a.render_desc(8, 8, 10, 3, hero_wavelengths=4)), UNS, "one wavelength per path"),
        "medium": (dict(rd=a.render_desc(8, 8, 10, 3, medium_aware=True)), UNS, "medium-aware walk"),
        "range": (dict(rd=a.render_desc(8, 8, 20, 3, first_sample=10, sample_count=10)), UNS, "whole sample range"),
        "shard2": (dict(rd=a.render_desc(8, 8, 10, 3, shard=(0, 2))), INV, "deals the tiles itself: shard_count must be 0"),
        "shard1": (dict(rd=a.render_desc(8, 8, 10, 3, shard=(0, 1))), INV, "deals the tiles itself: shard_count must be 0"),
    }
    for check in (fixed, adaptive):
        for key, (kw, status, word) in shared.items():
            assert check(check.__name__ + "_" + key, **kw) == status, (check.__name__, key)
    assert adaptive("adaptive_ad", null_ad=True) == INV
    assert adaptive("adaptive_counts", c=None) == INV
    assert adaptive("adaptive_tens", rd=a.render_desc(8, 8, 15, 3)) == INV
    assert adaptive("adaptive_below", ad=a.AdaptiveDesc(10, 10, 0.1, 0.0), rd=a.render_desc(8, 8, 20, 3)) == INV
    assert adaptive("adaptive_rel", ad=a.AdaptiveDesc(30, 10, -1.0, 0.0)) == INV
    assert adaptive("adaptive_phase", rd=a.render_desc(8, 8, 10, 3, phase_samples=5)) == UNS
    assert fixed("fixed_size", rd=a.render_desc(0, 8, 10, 3)) == INV
    assert fixed("fixed_camera", rd=a.render_desc(8, 8, 10, 3, camera_index=1)) == INV
    assert all(len(v) == 1 for v in msgs.values()), msgs
    flat = {k: next(iter(v))[1] for k, v in msgs.items()}
    for key, (kw, status, word) in shared.items():
        assert word in flat["fixed_" + key] and word in flat["adaptive_" + key], (key, flat["fixed_" + key])
        if not key.startswith("shard"):                                                  # the same rule, the same words in both entries ...
            assert flat["fixed_" + key] == flat["adaptive_" + key], key
        if "rd" in kw or "gd" in kw:                                                      # ... and, but for the shard, the one-device check's status and words
            st1, m1 = one(**{k: v for k, v in kw.items() if k in ("rd", "gd")})
            if key.startswith("shard"):
                assert (st1, m1) == ((UNS, "light groups render the whole film (shard_count 0 or 1)") if key == "shard2" else (PT_OK, m1))
            else:
                assert (st1, m1) == (status, flat["fixed_" + key]), key
    assert flat["fixed_shard2"] == "pt_render_light_groups_multi deals the tiles itself: shard_count must be 0"
    assert flat["adaptive_shard2"] == "pt_render_adaptive_light_groups_multi deals the tiles itself: shard_count must be 0"
    own = [flat["fixed_" + k] for k in shared if k not in ("g9", "shard1")] + \
          [flat["adaptive_" + k] for k in ("ad", "counts", "tens", "below", "rel", "phase", "shard2")] + [flat["fixed_size"], flat["fixed_camera"]]
    assert len(set(own)) == len(own), flat
    assert flat["adaptive_below"] == "max_samples < spp" and "sample_counts" in flat["adaptive_counts"] and "multiples of 10" in flat["adaptive_tens"]
    # the product runs the same checks before it looks for a device: without one (and so without a scene) the first of them is the one that can be seen
    L = pkg.load()
    rd, gd, ad = a.render_desc(8, 8, 10, 3), gdesc(), a.AdaptiveDesc(30, 10, 0.1, 0.0)
    assert L._render_light_groups_multi(None, C.byref(rd), C.byref(gd), 0, film.ctypes.data_as(f32p), None, None) == INV
    assert L.last_error() == flat["fixed_scene"]
    assert L._render_adaptive_light_groups_multi(None, C.byref(rd), C.byref(ad), C.byref(gd), 0, film.ctypes.data_as(f32p), counts.ctypes.data_as(u32p), None, None,
                                                 None) == INV
    assert L.last_error() == flat["fixed_scene"]


def test_ptcli_refuses_bad_light_group_devices_while_parsing(pkg, tmp_path):
    """Each refusal exits with status 2 and its own message before any file is read; the refusals of --devices with the two group flags stay what they were."""
    exe = ptcli(pkg)
    lg, dlg = ["--light-groups", "instance"], ["--denoise", "--denoise-light-groups", "instance"]
    cases = [
        (["--light-group-devices", "1"], "--light-group-devices needs --light-groups or --denoise-light-groups"),
        (["--denoise", "--light-group-devices", "1"], "--light-group-devices needs --light-groups or --denoise-light-groups"),
        (["--relamp-groups", "instance", "--relamp-bins", "4", "--light-group-devices", "1"], "--light-group-devices needs --light-groups or --denoise-light-groups"),
        (lg + ["--light-group-devices", "1", "--devices", "1"], "--light-group-devices cannot be combined with --devices"),
        (dlg + ["--devices", "1", "--light-group-devices", "1"], "--light-group-devices cannot be combined with --devices"),
        (lg + ["--light-group-devices", "x"], "--light-group-devices needs a device mask"),
        (lg + ["--light-group-devices", "3q"], "--light-group-devices needs a device mask"),
        (lg + ["--light-group-devices"], "--light-group-devices needs a value"),
        (dlg + ["--light-group-devices", "1", "--denoise-resident"], "--denoise-resident cannot be combined with --light-group-devices"),
        # the existing refusals, word for word
        (lg + ["--devices", "1"], "--light-groups cannot be combined with --devices: a group render is one plain render of one wavelength per path on one device"),
        (dlg + ["--devices", "1"], "--denoise-light-groups cannot be combined with --devices: it is one adaptive group render of one wavelength per path on one device, and its filter"),
        (dlg + ["--denoise-assemble"], "--denoise-light-groups cannot be combined with --denoise-assemble: it is one adaptive group render of one wavelength per path on one device, and its filter"),
        (lg + ["--light-group-devices", "1", "--denoise-assemble"], "--denoise-assemble needs --denoise"),
    ]
    seen = set()
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
        seen.add(message)
    assert len(seen) == 9
    assert "[--light-group-devices MASK]" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    head = open(os.path.join(CSRC, "host", "ptcli.cpp")).read().split("#include")[0]
    assert "[--light-group-devices MASK]" in head
    # dry runs with the flag parse and end well, --denoise-assemble beside it too
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    for args in (lg + ["--light-group-devices", "0x1"], dlg + ["--light-group-devices", "1"], dlg + ["--light-group-devices", "1", "--denoise-assemble"]):
        ok = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n"] + args, capture_output=True, text=True,
                            cwd=str(tmp_path))
        assert ok.returncode == 0 and re.search(r"light groups: \d+ ", ok.stdout), (args, ok.stdout, ok.stderr)


def test_sanitize_program_packs_scatters_and_unpacks_in_exact_buffers(tmp_path):
    """tools/shard_sanitize.cpp, a stand-alone host binary built with the address and undefined-behaviour sanitizers: the tests' films, shard counts
    and group counts in heap buffers of exactly the engine's sizes."""
    exe = str(tmp_path / "light_groups_shard_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tools", "shard_sanitize.cpp"), os.path.join(CSRC, "pt_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and r.stdout.count("every bit back") == 4 and not r.stderr, (r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------------ GPU tier
def room_rd(pkg, w=W, h=H, spp=20):
    return pkg.api.render_desc(w, h, spp, 5, light_samples=2, seed=7)


def tuned_scene(engine, pkg, builder, virt=0, rccl=False, batch_slots=0):
    t = clean_tuning(engine, pkg, batch_slots)
    t.multi_virtual = virt
    t.flags &= ~pkg.api.TUNE_MULTI_RCCL
    if rccl:
        t.flags |= pkg.api.TUNE_MULTI_RCCL
    return engine.create_scene(builder, t)


def counters(p):
    return [getattr(p, c) for c in COUNTERS]


def same_fixed(got, ref, what):
    """(film, group_films, profile)"""
    assert np.array_equal(bits(got[0]), bits(ref[0])), what
    assert got[1].shape == ref[1].shape and np.array_equal(bits(got[1]), bits(ref[1])), what
    assert counters(got[2]) == counters(ref[2]), what


def same_adaptive(got, ref, what):
    """(film, counts, stats, group_films, profile)"""
    assert np.array_equal(got[1], ref[1]), what
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64)), what
    assert np.array_equal(bits(got[0]), bits(ref[0])), what
    assert got[3].shape == ref[3].shape and np.array_equal(bits(got[3]), bits(ref[3])), what
    g, r = got[4], ref[4]
    assert g.kernel_launches[5] == r.kernel_launches[5], what
    assert g.camera_rays == r.camera_rays == int(ref[1].sum()), what
    assert counters(g) == counters(r), what


def random_matrices(seed, G):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (G, 3, 3)).astype(F)


@pytest.fixture(scope="module")
def room_ref(engine, pkg):
    """The one-device renders the node entries are compared with, made once: the fixed group render of the room at 77 x 45, 20 spp, and the adaptive one, 10 to 40
    spp in steps of 10 with a target between the pixels' own errors."""
    builder = pkg.scene.light_groups_room()
    sc = engine.create_scene(builder, clean_tuning(engine, pkg))
    fixed = sc.render_light_groups(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP)
    assert all(float(fixed[1][g][..., :3].max()) > 0.0 for g in range(3))
    rda = room_rd(pkg, spp=10)
    rel = pick_rel(engine, builder, rda, 0.4)
    adaptive = sc.render_adaptive_light_groups(rda, 40, rel, ROOM_GROUPS, ROOM_ENV_GROUP, step=10, stats=True)
    assert adaptive[1].min() < adaptive[1].max(), np.unique(adaptive[1])
    assert adaptive[4].kernel_launches[5] > 1
    return {"builder": builder, "fixed": fixed, "adaptive": adaptive, "rel": rel, "rda": rda}


def adaptive_node(sc, ref, **kw):
    return sc.render_adaptive_light_groups_multi(ref["rda"], 40, ref["rel"], ROOM_GROUPS, ROOM_ENV_GROUP, step=10, stats=True, device_mask=1, **kw)


@pytest.mark.gpu
def test_gpu_virtual_devices_equal_render_light_groups(engine, pkg, room_ref):
    """pt_render_light_groups_multi on the room, 77 x 45, 20 spp, 5 bounces, L = 2, seed 7, every emitter a group of its own, with multi_virtual 2, 3, 4, 4 with the
    RCCL path forced, and the RCCL path alone (one shard that is the whole film): film and group films as u32 and the five ray counters are
    pt_render_light_groups'.  Once more with batch_slots 2048: several passes per shard, both buffer sets of the overlap reused."""
    rd = room_rd(pkg)
    for virt, rccl, batch in ((2, False, 0), (3, False, 0), (4, False, 0), (4, True, 0), (0, True, 0), (3, False, 2048)):
        got = tuned_scene(engine, pkg, room_ref["builder"], virt, rccl, batch).render_light_groups_multi(rd, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)
        same_fixed(got, room_ref["fixed"], (virt, rccl, batch))


@pytest.mark.gpu
def test_gpu_environment_routing_crosses_shards(engine, pkg):
    """hdri_emissive_mesh with its second light (test_light_groups.emissive_mesh_scene: an importance-sampled environment, an emissive mesh and a rect lamp, a group
    each) on a 48 x 40 film of four tiles over three devices: pt_render_light_groups' bits."""
    b = emissive_mesh_scene(pkg)
    n = len(b.instances)
    three = [0] * n
    three[n - 2], three[n - 1] = 1, 2
    rd = pkg.api.render_desc(48, 40, 12, 5, light_samples=2, seed=3)
    ref = engine.create_scene(b, clean_tuning(engine, pkg)).render_light_groups(rd, three, 0)
    assert all(float(ref[1][g][..., :3].max()) > 0.0 for g in range(3))
    same_fixed(tuned_scene(engine, pkg, b, 3).render_light_groups_multi(rd, three, 0, device_mask=1), ref, "emissive mesh")


@pytest.mark.gpu
def test_gpu_empty_shards_eight_groups_and_no_read_back(engine, pkg, room_ref):
    """40 x 20 with multi_virtual 8: two tiles, six devices without a pixel.  G = 8 on the 77 x 45 film.  read_groups False: the same film, no group films on the
    host, and the resident mix of the shards is the mix of the films a reading call returned."""
    builder = room_ref["builder"]
    one = engine.create_scene(builder, clean_tuning(engine, pkg))
    small = room_rd(pkg, 40, 20)
    node8 = tuned_scene(engine, pkg, builder, 8)
    same_fixed(node8.render_light_groups_multi(small, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1), one.render_light_groups(small, ROOM_GROUPS, ROOM_ENV_GROUP), "8 devices, 2 tiles")
    assert node8.light_groups_resident() == (40, 20, 3)
    M = random_matrices(5, 3)
    assert np.array_equal(bits(node8.light_groups_mix_resident(M)), bits(engine.light_groups_mix(one.render_light_groups(small, ROOM_GROUPS, ROOM_ENV_GROUP)[1], M)))
    rd = room_rd(pkg)
    ids8 = (0, 1, 2, 3, 4, 5)
    ref8 = one.render_light_groups(rd, ids8, 7, groups=8)
    node = tuned_scene(engine, pkg, builder, 3)
    same_fixed(node.render_light_groups_multi(rd, ids8, 7, groups=8, device_mask=1), ref8, "8 groups")
    film, none, prof = node.render_light_groups_multi(rd, ids8, 7, groups=8, read_groups=False, device_mask=1)
    assert none is None and np.array_equal(bits(film), bits(ref8[0])) and counters(prof) == counters(ref8[2])
    assert node.light_groups_resident() == (W, H, 8)
    M8 = random_matrices(6, 8)
    assert np.array_equal(bits(node.light_groups_mix_resident(M8)), bits(engine.light_groups_mix(ref8[1], M8)))


@pytest.mark.gpu
def test_gpu_virtual_devices_equal_render_adaptive_light_groups(engine, pkg, room_ref):
    """pt_render_adaptive_light_groups_multi, 77 x 45, 10 to 40 spp in steps of 10 with counts that differ between pixels, multi_virtual 2, 3, 8 and 4 with RCCL
    forced: film, counts, stats, group films, rounds and the ray counters are pt_render_adaptive_light_groups'."""
    for virt, rccl in ((2, False), (3, False), (8, False), (4, True)):
        got = adaptive_node(tuned_scene(engine, pkg, room_ref["builder"], virt, rccl), room_ref)
        same_adaptive(got, room_ref["adaptive"], (virt, rccl))


@pytest.mark.gpu
def test_gpu_node_resident_mix(engine, pkg, room_ref):
    """After either entry the resident group films are the packed shards: pt_light_groups_resident tells their size, pt_light_groups_mix_resident is
    pt_light_groups_mix of the returned array bit for bit; a later one-device group render at another size replaces them, a node render after it is resident
    again; a refused node call leaves none; the denoised mix refuses after a node render without an assemble."""
    a = pkg.api
    sc = tuned_scene(engine, pkg, room_ref["builder"], 3)
    rd = room_rd(pkg)
    assert sc.light_groups_resident() is None
    _, groups, _ = sc.render_light_groups_multi(rd, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)
    assert sc.light_groups_resident() == (W, H, 3)
    for seed in (1, 2):
        M = random_matrices(seed, 3)
        got = sc.light_groups_mix_resident(M)
        assert got.shape == (H, W, 4) and np.any(got != 0)
        assert np.array_equal(bits(got), bits(engine.light_groups_mix(groups, M))), seed
    # the adaptive entry, another number of groups
    _, _, _, groups_a, _ = sc.render_adaptive_light_groups_multi(room_ref["rda"], 40, room_ref["rel"], (0, 1, 0, 0, 0, 0), 0, groups=2, step=10, stats=True, device_mask=1)
    assert sc.light_groups_resident() == (W, H, 2)
    M = random_matrices(3, 2)
    assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(groups_a, M)))
    assert sc.light_groups_denoised_resident() is None
    with pytest.raises(a.PtError, match="no resident denoised group films"):
        sc.light_groups_mix_resident(M, denoised=True)
    with pytest.raises(a.PtError, match="no resident film"):
        sc.denoise_light_groups_resident()
    # a one-device group render at another size replaces the resident films
    rd2 = a.render_desc(17, 13, 10, 4, light_samples=1, seed=2)
    _, groups2, _ = sc.render_light_groups(rd2, ROOM_GROUPS, ROOM_ENV_GROUP)
    assert sc.light_groups_resident() == (17, 13, 3)
    M = random_matrices(4, 3)
    assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(groups2, M)))
    # and a node render after it is resident again
    _, groups, _ = sc.render_light_groups_multi(rd, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)
    assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(groups, M)))
    # a node call that fails in its checks: no resident group films afterwards
    for refused in (lambda: sc.render_light_groups_multi(a.render_desc(W, H, 20, 5, seed=7, shard=(0, 2)), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1),
                    lambda: sc.render_light_groups_multi(rd, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1 << 40),
                    lambda: sc.render_adaptive_light_groups_multi(a.render_desc(W, H, 15, 5, seed=7), 30, 0.05, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)):
        sc.render_light_groups_multi(rd, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)
        assert sc.light_groups_resident() == (W, H, 3)
        with pytest.raises(a.PtError):
            refused()
        assert sc.light_groups_resident() is None
        with pytest.raises(a.PtError, match="no resident group films"):
            sc.light_groups_mix_resident(M)


@pytest.mark.gpu
@pytest.mark.parametrize("groups_first", [False, True], ids=["spectral_then_groups", "groups_then_spectral"])
def test_gpu_spectral_and_group_shards_of_two_film_sizes_stay_resident_together(engine, pkg, room_ref, groups_first):
    """One scene, four virtual devices: pt_render_spectral_multi at 40 x 20 with 5 bins and pt_render_light_groups_multi at 77 x 45 with G = 3, in either order.
    Both stay resident, each in shards with pixel lists of its own film: pt_spectral_project_resident with a 2 x 5 matrix is pt_spectral_project of the bins the
    spectral call returned, and pt_light_groups_mix_resident is pt_light_groups_mix of the group films the group call returned, both bit for bit."""
    sc = tuned_scene(engine, pkg, room_ref["builder"], 4)
    out = {}
    for groups in (groups_first, not groups_first):
        if groups:
            out["groups"] = sc.render_light_groups_multi(room_rd(pkg, spp=4), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)[1]
        else:
            out["bins"] = sc.render_spectral_multi(room_rd(pkg, 40, 20, spp=4), 5, device_mask=1)[1]
    assert sc.spectral_resident() == (40, 20, 5) and sc.light_groups_resident() == (W, H, 3)
    assert np.any(out["bins"] != 0) and np.any(out["groups"] != 0)
    K = np.random.default_rng(21).uniform(-1.0, 1.0, (2, 5)).astype(F)
    M = random_matrices(22, 3)
    assert np.array_equal(bits(sc.spectral_project_resident(K)), bits(engine.spectral_project(out["bins"], K)))
    assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(out["groups"], M)))


@pytest.fixture(scope="module")
def one_device_filtered(engine, pkg, room_ref):
    """The one-device sequence the assembled one is compared with: the adaptive group render, resident guides with the albedo, the joint filter, the relight of
    the denoised group films."""
    sc = engine.create_scene(room_ref["builder"], clean_tuning(engine, pkg))
    film, counts, st, groups, _ = sc.render_adaptive_light_groups(room_ref["rda"], 40, room_ref["rel"], ROOM_GROUPS, ROOM_ENV_GROUP, step=10, stats=True)
    sc.resident_guides(room_ref["rda"], 4, 0, albedo=True)
    den, den_groups = sc.denoise_light_groups_resident()
    M = random_matrices(9, 3)
    return {"film": film, "counts": counts, "stats": st, "groups": groups, "den": den, "den_groups": den_groups, "M": M,
            "relit": sc.light_groups_mix_resident(M, denoised=True), "noisy_relit": sc.light_groups_mix_resident(M)}


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [False, True], ids=["in_place", "staged"])
def test_gpu_assemble_then_filter_and_relight(engine, pkg, room_ref, one_device_filtered, staged):
    """After the adaptive node entry: resident_assemble (once with every shard staged), resident_guides, denoise_light_groups_resident and the denoised relight.
    Film, denoised film, denoised group films and relight equal the one-device sequence bit for bit; resident_read returns the assembled film."""
    a = pkg.api
    want = one_device_filtered
    sc = tuned_scene(engine, pkg, room_ref["builder"], 3)
    got = adaptive_node(sc, room_ref)
    same_adaptive(got, room_ref["adaptive"], staged)
    assert sc.resident_info()[3] == 0
    sc.resident_assemble(staged=staged)
    assert sc.resident_info()[:2] == (W, H) and sc.resident_info()[3] & a.RESIDENT_FILM and sc.light_groups_resident() == (W, H, 3)
    film, counts, st = sc.resident_read()
    assert np.array_equal(bits(film), bits(want["film"])) and np.array_equal(counts, want["counts"]) and np.array_equal(st.view(np.uint64), want["stats"].view(np.uint64))
    assert np.array_equal(bits(sc.light_groups_mix_resident(want["M"])), bits(want["noisy_relit"]))      # (the unpacked films, on the scene's device)
    sc.resident_guides(room_ref["rda"], 4, 0, albedo=True)
    den, den_groups = sc.denoise_light_groups_resident()
    assert np.array_equal(bits(den), bits(want["den"])) and np.array_equal(bits(den_groups), bits(want["den_groups"]))
    assert not np.array_equal(bits(den_groups), bits(want["groups"]))
    assert np.array_equal(bits(sc.light_groups_mix_resident(want["M"], denoised=True)), bits(want["relit"]))
    # the Python route: the mask with and without the assemble gives the one-device outputs
    if not staged:
        for assemble in (False, True):
            out = tuned_scene(engine, pkg, room_ref["builder"], 2).render_denoised_light_groups(
                room_ref["rda"], ROOM_GROUPS, ROOM_ENV_GROUP, max_samples=40, rel_error=room_ref["rel"], step=10, albedo=True, device_mask=1, assemble=assemble)
            for g, w_ in zip(out[:4], (want["film"], want["den"], want["groups"], want["den_groups"])):
                assert np.array_equal(bits(g), bits(w_)), assemble
            assert np.array_equal(out[4], want["counts"])


@pytest.mark.gpu
def test_gpu_assemble_after_a_node_render_without_groups_is_what_it_was(engine, pkg, room_ref):
    """pt_resident_assemble after pt_render_adaptive_multi: the arrays that render returned, through resident_read; group films an earlier node group render left
    in shards stay resident and unpaired."""
    a = pkg.api
    sc = tuned_scene(engine, pkg, room_ref["builder"], 3)
    _, groups, _ = sc.render_light_groups_multi(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)
    film, counts, st, _ = sc.render_adaptive_multi(room_ref["rda"], 40, room_ref["rel"], step=10, stats=True, device_mask=1)
    assert np.array_equal(bits(film), bits(room_ref["adaptive"][0]))
    sc.resident_assemble()
    assert sc.resident_info() == (W, H, 0, a.RESIDENT_FILM)
    rf, rc, rs = sc.resident_read()
    assert np.array_equal(bits(rf), bits(film)) and np.array_equal(rc, counts) and np.array_equal(rs.view(np.uint64), st.view(np.uint64))
    assert sc.light_groups_resident() == (W, H, 3)
    M = random_matrices(12, 3)
    assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(groups, M)))
    sc.resident_guides(room_ref["rda"], 4, 0)
    with pytest.raises(a.PtError, match="no group films of the resident film's render"):
        sc.denoise_light_groups_resident()


@pytest.mark.gpu
def test_gpu_state_across_calls(engine, pkg, room_ref):
    """A second call reuses the set-up (kernel_seconds[5] smaller than the first call's); the current device is kept; pt_render and pt_render_light_groups before
    and after a node group render on one handle give the same bits."""
    rd = room_rd(pkg)
    sc = tuned_scene(engine, pkg, room_ref["builder"], 4, rccl=True)
    before = _hip_current_device()
    plain0, pprof0 = sc.render(rd)
    one0 = sc.render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP)
    same_fixed(one0, room_ref["fixed"], "one device, before")
    setup = []
    for call in range(2):
        got = sc.render_light_groups_multi(rd, ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)
        same_fixed(got, room_ref["fixed"], call)
        assert got[2].seconds > 0 and got[2].kernel_seconds[6] > 0
        setup.append(got[2].kernel_seconds[5])
    assert setup[1] < setup[0], setup
    setup = []
    for call in range(2):
        got = adaptive_node(sc, room_ref)
        same_adaptive(got, room_ref["adaptive"], call)
        assert got[4].seconds > 0 and got[4].kernel_seconds[6] > 0
        setup.append(got[4].kernel_seconds[5])
    assert setup[1] < setup[0], setup   # (the first adaptive call found replicas, streams and films made, and made the adaptive buffers)
    sc.light_groups_mix_resident(random_matrices(1, 3))
    assert _hip_current_device() == before
    plain1, pprof1 = sc.render(rd)
    assert np.array_equal(bits(plain1), bits(plain0)) and counters(pprof1) == counters(pprof0)
    same_fixed(sc.render_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP), one0, "one device, after")
    assert np.array_equal(bits(plain0), bits(room_ref["fixed"][0]))


@pytest.mark.gpu
def test_gpu_plain_masks_are_the_one_device_calls(engine, pkg, room_ref):
    """Masks 0 and 1 without virtual devices are the one-device renders (on a box with one GPU, mask 0 too), and leave the one-device resident state, pairing
    included; a mask naming no device is refused."""
    a = pkg.api
    if engine.lib.pt_device_count() > 1:
        masks = (1,)
    else:
        masks = (0, 1)
    sc = tuned_scene(engine, pkg, room_ref["builder"])
    for mask in masks:
        same_fixed(sc.render_light_groups_multi(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=mask), room_ref["fixed"], mask)
        got = sc.render_adaptive_light_groups_multi(room_ref["rda"], 40, room_ref["rel"], ROOM_GROUPS, ROOM_ENV_GROUP, step=10, stats=True, device_mask=mask)
        same_adaptive(got, room_ref["adaptive"], mask)
        assert sc.resident_info()[3] & a.RESIDENT_FILM
        sc.resident_guides(room_ref["rda"], 4, 0)
        den, den_groups = sc.denoise_light_groups_resident()      # (paired: the node.single branch is the one-device call)
        assert den_groups.shape == got[3].shape
    with pytest.raises(a.PtError, match="names no visible HIP device"):
        sc.render_light_groups_multi(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1 << 40)
    with pytest.raises(a.PtError, match="shard_count must be 0"):
        sc.render_light_groups_multi(a.render_desc(W, H, 20, 5, seed=7, shard=(0, 2)), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=1)


@pytest.mark.gpu
def test_gpu_two_physical_devices(engine, pkg, room_ref):
    """Masks 0b11 and 0b10 over two real devices equal the one-device render (runs only where the box has them)."""
    if engine.lib.pt_device_count() < 2:
        pytest.skip("one HIP device on this box")
    sc = tuned_scene(engine, pkg, room_ref["builder"])
    for mask in (0b11, 0b10):
        got = sc.render_light_groups_multi(room_rd(pkg), ROOM_GROUPS, ROOM_ENV_GROUP, device_mask=mask)
        same_fixed(got, room_ref["fixed"], mask)
        M = random_matrices(mask, 3)
        assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(got[1], M)))
        got = sc.render_adaptive_light_groups_multi(room_ref["rda"], 40, room_ref["rel"], ROOM_GROUPS, ROOM_ENV_GROUP, step=10, stats=True, device_mask=mask)
        same_adaptive(got, room_ref["adaptive"], mask)
        sc.resident_assemble()
        assert np.array_equal(bits(sc.light_groups_mix_resident(M)), bits(engine.light_groups_mix(got[3], M)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["light_groups", "denoise_light_groups"])
def test_gpu_ptcli_light_group_devices(pkg, tmp_path, mode):
    """ptcli with --light-group-devices 1 under PT_AMD_MULTI_VIRTUAL=3 (the node calls, three shards; the relight through the node-resident films) writes every file
    of the run without the flag, byte for byte; with --denoise-light-groups also with --denoise-assemble, the resident route."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]
    flags = ["--light-groups", "instance"] if mode == "light_groups" else ["--denoise", "--denoise-light-groups", "instance"]
    dry = subprocess.run(base + ["--output-dir", str(tmp_path / "dry"), "-n"] + flags, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    G = int(re.search(r"light groups: (\d+) ", dry.stdout).group(1))
    flags += ["--light-gains", ",".join(str(0.5 + 0.75 * g) for g in range(G))]
    node_env = {"PT_AMD_MULTI_VIRTUAL": "3"}
    runs = {"one": ([], {}), "node": (["--light-group-devices", "1"], node_env)}
    if mode == "denoise_light_groups":
        runs["assembled"] = (["--light-group-devices", "1", "--denoise-assemble"], node_env)
    for name, (extra, env) in runs.items():
        r = subprocess.run(base + ["--output-dir", str(tmp_path / name)] + flags + extra, capture_output=True, text=True, cwd=str(tmp_path), timeout=120,
                           env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(os.listdir(str(tmp_path / "one")))
    stem = "beauty"
    want = [stem + e for e in (".exr", ".png", "_relit.exr", "_relit.png")] + ["%s_light%d.exr" % (stem, g) for g in range(G)]
    if mode == "denoise_light_groups":
        want += [stem + e for e in ("_denoised.exr", "_denoised.png", "_denoised_relit.exr", "_denoised_relit.png")] + ["%s_denoised_light%d.exr" % (stem, g) for g in range(G)]
    assert files == sorted(want)
    for name in runs:
        assert sorted(os.listdir(str(tmp_path / name))) == files, name
        for f in files:
            assert (tmp_path / "one" / f).read_bytes() == (tmp_path / name / f).read_bytes(), (name, f)
