"""A node render assembled on one device for the resident filter (pt_resident_assemble and pt_resident_read, include/pt_resident.h, DESIGN.md section 14,
"Assembling a node render").  Everything is moved and nothing computed, so every comparison is bit for bit.  The CPU tier checks the unpack rule the kernel
compiles (csrc/pt_shard_rules.h, through tests/host_emulation/ptemu_resident_assemble.cpp) against a numpy restatement, the refusals of
pth::check_resident_assemble, the library's exports and bindings, and the refusals of the Python layer and of the command line.  The GPU tier renders on
virtual devices, assembles, and compares what pt_resident_read returns with the arrays the render returned, the filter on the assembled set with the filter
after pt_resident_load and with the host-array entry, walks the life of the remembered node render, and compares the Python routes and ptcli's files."""
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
from test_spectral import scaled_c2_config
from test_spectral_multi import BINS, FILMS, H, W, bits, np_shard_pixels, random_planes, tuned_scene
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED, PT_OK, ptcli

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
u32p, f32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
F = np.float32
SHARDS = (1, 2, 3, 4, 8)          # the shard counts of tests/test_spectral_multi.py
CPU_BINS = (1, 5, 13, 64)
NO_NODE_RENDER = "no node render to assemble"
WITHOUT_STATS = "made without stats"


@pytest.fixture(scope="session")
def emu_as(pkg):
    """The unpack rule and pt_resident_assemble's checks on the host, beside the pack rule and the shard lists (ptemu_spectral_shard.cpp): a library of its own."""
    L = C.CDLL(emulation.library_path("resident_assemble"))
    L.ptemu_resident_assemble_last_error.restype = C.c_char_p
    L.ptemu_shard_pixels.restype = C.c_uint32
    L.ptemu_shard_pixels.argtypes = [C.c_uint32] * 6 + [C.c_void_p, C.c_uint32]
    L.ptemu_spectral_shard_pack.restype = None
    L.ptemu_spectral_shard_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.ptemu_spectral_shard_unpack.restype = None
    L.ptemu_spectral_shard_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    L.ptemu_resident_assemble_check.restype = C.c_int32
    L.ptemu_resident_assemble_check.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    return L


# ------------------------------------------------------------------------------------------------ CPU tier
def np_unpack(packed, px, planes):
    """shard_unpack_item for every item: planes[b, px[i]] = packed[b, i]"""
    planes[:, px] = packed


@pytest.mark.parametrize("tile", (32, 8))
@pytest.mark.parametrize("w,h", FILMS)
def test_unpack_equals_its_numpy_restatement_and_writes_every_float_once(emu_as, w, h, tile):
    """For every film, tile size (32, the renders', and 8: many tiles per shard) and shard count of tests/test_spectral_multi.py and B = 1, 5, 13, 64 over
    planes of random bit patterns (NaN payloads, a NaN with a clear quiet bit and -0.0 among them): the emulation's unpack of one shard into a sentinel
    destination is the numpy restatement's, and touches no other float; every shard of a pack unpacked in reversed order returns the planes bit for bit; the
    sentinel of every float is replaced exactly once — a float written twice would show in the per-shard comparison, where everything outside the shard's own
    pixels still holds the sentinel.  With 8 shards of 32 x 32 tiles on 40 x 20, six shards are empty."""
    npx = w * h
    SENTINEL = 0xDEADBEEF
    for n in SHARDS:
        lists = []
        for v in range(n):
            index, count = (v, n) if n > 1 else (0, 0)
            px = np.zeros(npx, np.uint32)
            k = emu_as.ptemu_shard_pixels(w, h, tile, tile, index, count, px.ctypes.data, npx)
            assert np.array_equal(px[:k], np_shard_pixels(w, h, tile, tile, index, count)), (n, v)
            lists.append(px[:k].copy())
        if (w, h, n, tile) == (40, 20, 8, 32):
            assert sorted(len(px) for px in lists) == [0] * 6 + [8 * 20, 32 * 20]
        for B in CPU_BINS:
            rng = np.random.default_rng(100000 * w + 1000 * n + 10 * B + tile)
            planes = random_planes(rng, B, npx)
            planes[planes == SENTINEL] = 0                                               # (so that the sentinel stands for "not written" alone)
            back = np.full((B, npx), SENTINEL, np.uint32)
            writes = np.zeros((B, npx), np.int64)
            for px in reversed(lists):
                k = px.size
                if not k:                                                                 # (a shard without a pixel moves nothing and launches nothing)
                    continue
                packed = np.full((B, k), 0xABABABAB, np.uint32)
                emu_as.ptemu_spectral_shard_pack(planes.ctypes.data, npx, px.ctypes.data, k, B, packed.ctypes.data)
                alone, want = np.full((B, npx), SENTINEL, np.uint32), np.full((B, npx), SENTINEL, np.uint32)
                emu_as.ptemu_spectral_shard_unpack(packed.ctypes.data, px.ctypes.data, k, B, alone.ctypes.data, npx)
                np_unpack(packed, px, want)
                assert np.array_equal(alone, want), (n, B)
                writes += alone != SENTINEL                                               # the floats this shard wrote: its own pixels' and no other
                assert int((alone != SENTINEL).sum()) == B * k, (n, B)
                emu_as.ptemu_spectral_shard_unpack(packed.ctypes.data, px.ctypes.data, k, B, back.ctypes.data, npx)
            assert np.array_equal(back, planes), (n, B)
            assert np.array_equal(writes, np.ones((B, npx), np.int64)), (n, B)
            if npx > 2:
                assert back.reshape(-1)[0] == 0x80000000 and back.reshape(-1)[-1] == 0x7FC12345 and back.reshape(-1)[back.size // 2] == 0xFF800001


def test_assemble_refuses_each_bad_call_with_its_own_message(emu_as, pkg):
    """check_resident_assemble through the emulation, then the product's entries, which run their checks before they look for a device."""
    scene = C.c_void_p(1)   # (only compared with null)
    got = {}

    def check(name, sc, flags, remembered, stats, want=PT_ERR_INVALID_ARGUMENT):
        st = emu_as.ptemu_resident_assemble_check(sc, flags, remembered, stats, W, H, BINS)
        assert st == want, name
        if st != PT_OK:
            got[name] = emu_as.ptemu_resident_assemble_last_error().decode()
    check("ok", scene, 0, 1, 1, PT_OK)
    check("ok_staged", scene, pkg.api.RESIDENT_ASSEMBLE_STAGED, 1, 1, PT_OK)
    check("scene", None, 0, 1, 1)
    check("flags", scene, 2, 1, 1)
    check("flags_high", scene, 1 << 31 | 1, 1, 1)
    check("nothing", scene, 0, 0, 0)
    check("nothing_stats", scene, 0, 0, 1)
    check("no_stats", scene, 0, 1, 0)
    assert got["flags"] == got["flags_high"] and got["nothing"] == got["nothing_stats"]
    own = [got[k] for k in ("scene", "flags", "nothing", "no_stats")]
    assert len(set(own)) == 4 and all(m.startswith("pt_resident_assemble: ") for m in own), got
    assert "scene is null" in got["scene"] and "PT_RESIDENT_ASSEMBLE_STAGED" in got["flags"] and NO_NODE_RENDER in got["nothing"] and WITHOUT_STATS in got["no_stats"]
    # the product: without a device there is no scene to make, so the null scene is the refusal that can be seen
    L = pkg.load()
    assert L._resident_assemble(None, 0) == PT_ERR_INVALID_ARGUMENT and L.last_error() == got["scene"]
    assert L._resident_read(None, None, None, None, None) == PT_ERR_INVALID_ARGUMENT
    assert "pt_resident_read" in L.last_error() and "scene is null" in L.last_error()


def test_library_exports_the_entries_and_the_bindings_mirror_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    a = pkg.api
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pt_resident.h")).read(), flags=re.S)

    def header_types(name):
        params = re.search(r"pt_status\s+%s\s*\((.*?)\);" % name, text, re.S).group(1)
        return [re.sub(r"\s+", " ", p.strip().rsplit(" ", 1)[0].replace("*", " *")).replace(" *", "*") for p in params.split(",")]
    L = a.Library(pkg.LIBRARY_PATH)
    cases = {
        "resident_assemble": (["pt_scene*", "uint32_t"], [C.c_void_p, C.c_uint32]),
        "resident_read": (["pt_scene*", "float*", "uint32_t*", "double*", "float*"], [C.c_void_p, f32p, u32p, f64p, f32p]),
    }
    for name, (types, want) in cases.items():
        assert hasattr(lib, "pt_" + name), name
        assert name not in a.API_FUNCTIONS   # (pt_resident.h, not the oracle's boundary)
        assert header_types("pt_" + name) == types, name
        fn = getattr(L, "_" + name)
        assert fn is not None and list(fn.argtypes) == want and fn.restype == C.c_int32, name
    assert int(re.search(r"#define\s+PT_RESIDENT_ASSEMBLE_STAGED\s+(\d+)u", text).group(1)) == a.RESIDENT_ASSEMBLE_STAGED
    assert inspect.signature(a.Scene.resident_assemble).parameters["staged"].default is False
    read = inspect.signature(a.Scene.resident_read).parameters
    assert [(k, p.default) for k, p in read.items() if k != "self"] == [("film", True), ("counts", True), ("stats", True), ("spectral", False)]
    for method in (a.Scene.render_denoised, a.Scene.render_denoised_spectral):
        assert inspect.signature(method).parameters["assemble"].default is False


class _NoCalls:
    """A library that must not be called: the refusal comes before anything is rendered."""
    path, prefix = "none", "pt_"

    def __getattr__(self, name):
        raise AssertionError("the layer called %s before refusing" % name)


def test_python_refuses_assemble_without_a_device_mask(pkg):
    a = pkg.api
    sc = a.Scene.__new__(a.Scene)
    sc.library, sc.handle = _NoCalls(), None
    rd = a.render_desc(8, 8, 10, 4)
    messages = set()
    for call in (lambda: sc.render_denoised(rd, 20, 0.05, assemble=True), lambda: sc.render_denoised_spectral(rd, 5, 20, 0.05, assemble=True),
                 lambda: sc.render_denoised_spectral(rd, 5, 20, 0.05, assemble=True, resident=True)):
        with pytest.raises(a.PtError, match="assemble=True needs a device_mask") as e:
            call()
        assert e.value.status == PT_ERR_UNSUPPORTED
        messages.add(str(e.value))
    assert len(messages) == 2   # (each method names itself)
    # the refusals of resident=True with a device_mask stay what they were, with or without the new keyword
    for kw in (dict(), dict(assemble=True)):
        with pytest.raises(a.PtError, match=r"render_denoised: resident=True takes no device_mask \(a node render leaves no film one device can filter\)"):
            sc.render_denoised(rd, 20, 0.05, resident=True, device_mask=1, **kw)
        with pytest.raises(a.PtError, match=r"render_denoised_spectral: resident=True takes no device_mask \(a node render leaves no film one device can filter\)"):
            sc.render_denoised_spectral(rd, 5, 20, 0.05, resident=True, device_mask=1, **kw)


def test_ptcli_refuses_bad_denoise_assemble_while_parsing(pkg, tmp_path):
    """Each refusal exits with status 2 and its own message before any file is read; --help and the head of the source list the flag; a dry run with it parses."""
    exe = ptcli(pkg)
    full = ["--denoise", "--denoise-spectral-bins", "8", "--spectral-devices", "1"]
    cases = [
        (["--denoise-assemble"], "--denoise-assemble needs --denoise"),
        (["--denoise", "--denoise-assemble"], "--denoise-assemble needs --denoise-spectral-bins"),
        (["--denoise", "--denoise-spectral-bins", "8", "--denoise-assemble"], "--denoise-assemble needs --spectral-devices"),
        (["--denoise", "--denoise-assemble", "--devices", "1"], "--denoise-assemble needs --denoise-spectral-bins"),
        (["--spectral-bins", "8", "--spectral-devices", "1", "--denoise-assemble"], "--denoise-assemble needs --denoise"),
        (["--denoise", "--denoise-spectral-bins", "8", "--denoise-resident", "--denoise-assemble"], "--denoise-assemble cannot be combined with --denoise-resident"),
        # an existing refusal comes first, word for word
        (full + ["--denoise-resident", "--denoise-assemble"], "--denoise-resident cannot be combined with --spectral-devices: a node render leaves no film one device can filter"),
    ]
    seen = set()
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
        seen.add(message)
    assert len(seen) == 5
    assert "[--denoise-assemble]" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    head = open(os.path.join(CSRC, "host", "ptcli.cpp")).read().split("#include")[0]
    assert "[--denoise-assemble]" in head
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    ok = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n"] + full + ["--denoise-assemble"],
                        capture_output=True, text=True, cwd=str(tmp_path))
    assert ok.returncode == 0, ok.stderr


# ------------------------------------------------------------------------------------------------ GPU tier
_REL = {}


def node_desc(engine, pkg, w=W, h=H):
    """The spectral multi tests' adaptive render: 10 to 40 spp in steps of 10, the target picked so that the counts differ between pixels (once per size)."""
    builder = pkg.scene.cornell_box()
    rd = pkg.api.render_desc(w, h, 10, 4, seed=7)
    if (w, h) not in _REL:
        _REL[(w, h)] = pick_rel(engine, builder, rd, 0.4)
    return builder, rd, _REL[(w, h)]


def node_render(sc, rd, rel, bins=BINS):
    """(film, counts, stats, spectral) of the adaptive spectral node render on the devices of mask 1"""
    film, counts, stats, spectral, _ = sc.render_adaptive_spectral_multi(rd, bins, 40, rel, step=10, stats=True, device_mask=1)
    return film, counts, stats, spectral


def assert_assembled(sc, arrays, what):
    """pt_resident_read of the assembled set against the arrays the render returned"""
    film, counts, stats, spectral = arrays
    got = sc.resident_read(spectral=spectral is not None)
    assert np.array_equal(bits(got[0]), bits(film)), (what, "film")
    assert np.array_equal(got[1], counts), (what, "counts")
    assert np.array_equal(got[2].view(np.uint64), stats.view(np.uint64)), (what, "stats")
    if spectral is not None:
        assert got[3].shape == spectral.shape and np.array_equal(bits(got[3]), bits(spectral)), (what, "bins: %d differ" % int((bits(got[3]) != bits(spectral)).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("virt,rccl", ((2, False), (3, False), (8, False), (4, True)))
def test_gpu_assembled_bits_equal_the_arrays_the_render_returned(engine, pkg, virt, rccl):
    """77 x 45, B = 5, virtual devices 2, 3, 8 and 4 with the RCCL path forced: film, counts, stats and bins, in place and staged; a second assemble of the same
    render gives the same bits; resident_info tells FILM | BINS with the size and the bins."""
    a = pkg.api
    builder, rd, rel = node_desc(engine, pkg)
    sc = tuned_scene(engine, pkg, builder, virt, rccl)
    arrays = node_render(sc, rd, rel)
    assert arrays[1].min() < arrays[1].max()
    assert sc.resident_info() == (0, 0, 0, 0)
    for staged in (False, True, False):
        sc.resident_assemble(staged=staged)
        assert sc.resident_info() == (W, H, BINS, a.RESIDENT_FILM | a.RESIDENT_BINS)
        assert_assembled(sc, arrays, (virt, rccl, staged))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", (13, 64))
def test_gpu_assembled_bits_with_more_bins(engine, pkg, B):
    builder, rd, rel = node_desc(engine, pkg)
    sc = tuned_scene(engine, pkg, builder, 3)
    arrays = node_render(sc, rd, rel, B)
    for staged in (False, True):
        sc.resident_assemble(staged=staged)
        assert sc.resident_info()[2] == B
        assert_assembled(sc, arrays, (B, staged))
    sc.close()


@pytest.mark.gpu
def test_gpu_empty_shards(engine, pkg):
    """40 x 20 on 8 virtual devices: two tiles, six shards without a pixel."""
    builder, rd, rel = node_desc(engine, pkg, 40, 20)
    sc = tuned_scene(engine, pkg, builder, 8)
    arrays = node_render(sc, rd, rel)
    for staged in (False, True):
        sc.resident_assemble(staged=staged)
        assert_assembled(sc, arrays, staged)
    sc.close()


@pytest.mark.gpu
def test_gpu_filter_on_the_assembled_set(engine, pkg):
    """Guides with both albedos and the joint filter on the assembled set: film, variance and bins equal the same calls after resident_load of the render's
    host arrays and denoise_spectral_albedo of those arrays; the denoised development is spectral_project of those bins; the undenoised, node-resident
    development gives the same planes before and after the assemble."""
    a = pkg.api
    builder, rd, rel = node_desc(engine, pkg)
    sc = tuned_scene(engine, pkg, builder, 3)
    film, counts, stats, spectral = node_render(sc, rd, rel)
    M = engine.spectral_observer_matrix(rd, BINS)
    before = sc.spectral_project_resident(M)
    assert np.array_equal(bits(before), bits(engine.spectral_project(spectral, M)))
    sc.resident_assemble()
    sc.resident_guides(rd, 4, albedo=True, bin_albedo=True)
    assert sc.resident_info() == (W, H, BINS, a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES | a.RESIDENT_ALBEDO | a.RESIDENT_BIN_ALBEDO)
    got = sc.denoise_resident(variance=True, spectral=True)
    developed = sc.spectral_project_resident(M, denoised=True)
    assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(before))
    # the host-array entry over what the render and the guide entry returned
    guides, alb, balb = sc.render_guides_bin_albedo(rd, BINS, 4)
    den, den_bins, var = engine.denoise_spectral_albedo(film, counts, stats, guides, spectral, alb, balb, variance=True)
    for g, w_, name in zip(got, (den, var, den_bins), ("film", "variance", "bins")):
        assert np.array_equal(bits(g), bits(w_)), ("host-array entry", name)
    assert np.array_equal(bits(developed), bits(engine.spectral_project(den_bins, M)))
    # the same calls after resident_load of the host arrays, on a scene of its own
    loaded = engine.create_scene(builder)
    loaded.resident_load(film, counts, stats, spectral=spectral)
    loaded.resident_guides(rd, 4, albedo=True, bin_albedo=True)
    for g, w_, name in zip(got, loaded.denoise_resident(variance=True, spectral=True), ("film", "variance", "bins")):
        assert np.array_equal(bits(g), bits(w_)), ("resident_load", name)
    # assembling again drops guides and denoised parts, as resident_load of a film does not keep what belonged to another
    sc.resident_assemble(staged=True)
    assert sc.resident_info()[3] == a.RESIDENT_FILM | a.RESIDENT_BINS
    loaded.close(); sc.close()


@pytest.mark.gpu
def test_gpu_without_bins(engine, pkg):
    """render_adaptive_multi then assemble: FILM alone, and denoise_resident is denoise_film."""
    a = pkg.api
    builder, rd, rel = node_desc(engine, pkg)
    sc = tuned_scene(engine, pkg, builder, 3)
    film, counts, stats, _ = sc.render_adaptive_multi(rd, 40, rel, step=10, stats=True, device_mask=1)
    assert sc.resident_info() == (0, 0, 0, 0)
    for staged in (False, True):
        sc.resident_assemble(staged=staged)
        assert sc.resident_info() == (W, H, 0, a.RESIDENT_FILM)
        assert_assembled(sc, (film, counts, stats, None), staged)
    with pytest.raises(a.PtError, match="pt_resident_read: spectral without resident bins"):
        sc.resident_read(spectral=True)
    sc.resident_guides(rd, 4)
    den, var = sc.denoise_resident(variance=True)
    want, want_var = engine.denoise_film(film, counts, stats, sc.render_guides(rd, 4), variance=True)
    assert np.array_equal(bits(den), bits(want)) and np.array_equal(bits(var), bits(want_var))
    sc.close()


@pytest.mark.gpu
def test_gpu_life_of_the_remembered_node_render(engine, pkg):
    """Nothing is resident right after the node render; the assemble makes FILM | BINS; any later render ends it and forgets the node render: a one-device
    render, a fixed-count node render, a node render made without stats and a failed node render each leave the assemble refused, with the message of their
    kind.  The caller's current device is unchanged; pt_resident_read reads a rendered set too."""
    a = pkg.api
    builder, rd, rel = node_desc(engine, pkg)
    sc = tuned_scene(engine, pkg, builder, 2)
    before = _hip_current_device()
    with pytest.raises(a.PtError, match=NO_NODE_RENDER):     # a fresh scene
        sc.resident_assemble()
    with pytest.raises(a.PtError, match="pt_resident_read: film_xyzw without a resident film"):
        sc.resident_read()
    assert sc.resident_read(film=False, counts=False, stats=False) is None   # (nothing asked for: nothing refused)
    arrays = node_render(sc, rd, rel)
    assert sc.resident_info() == (0, 0, 0, 0)
    sc.resident_assemble()
    assert sc.resident_info() == (W, H, BINS, a.RESIDENT_FILM | a.RESIDENT_BINS)
    assert_assembled(sc, arrays, "first")
    laters = {
        "one-device render": (lambda: sc.render(rd), NO_NODE_RENDER),
        "fixed-count node render": (lambda: sc.render_spectral_multi(rd, BINS, device_mask=1), NO_NODE_RENDER),
        "fixed-count node render without bins": (lambda: sc.render_multi(rd, device_mask=1), NO_NODE_RENDER),
        "node render without stats": (lambda: sc.render_adaptive_spectral_multi(rd, BINS, 40, rel, step=10, device_mask=1), WITHOUT_STATS),
    }
    for name, (later, message) in laters.items():
        node_render(sc, rd, rel)
        sc.resident_assemble()
        later()
        assert sc.resident_info() == (0, 0, 0, 0), name
        with pytest.raises(a.PtError, match=message):
            sc.resident_assemble()
        assert sc.resident_info() == (0, 0, 0, 0), name
    # a one-device adaptive render leaves its own film resident, and nothing to assemble
    one = sc.render_adaptive_spectral(rd, BINS, 40, rel, step=10, stats=True)
    assert sc.resident_info() == (W, H, BINS, a.RESIDENT_FILM | a.RESIDENT_BINS)
    assert_assembled(sc, (one[0], one[1], one[2], one[3]), "pt_resident_read of a rendered set")
    with pytest.raises(a.PtError, match=NO_NODE_RENDER):
        sc.resident_assemble()
    # failed node renders: refused in the checks, and a mask that names no device
    for failed in (lambda: sc.render_adaptive_spectral_multi(a.render_desc(W, H, 15, 4, seed=7), BINS, 30, 0.05, stats=True, device_mask=1),
                   lambda: sc.render_adaptive_spectral_multi(rd, BINS, 40, rel, step=10, stats=True, device_mask=1 << 40),
                   lambda: sc.render_adaptive_multi(rd, 40, rel, step=10, stats=True, device_mask=1 << 40)):
        node_render(sc, rd, rel)
        with pytest.raises(a.PtError):
            failed()
        with pytest.raises(a.PtError, match=NO_NODE_RENDER):
            sc.resident_assemble()
    # and after all that a node render assembles as the first did
    again = node_render(sc, rd, rel)
    sc.resident_assemble()
    assert_assembled(sc, again, "again")
    assert_assembled(sc, arrays, "the same render, the same bits")
    with pytest.raises(a.PtError, match="PT_RESIDENT_ASSEMBLE_STAGED"):
        sc.library.call("resident_assemble", sc.handle, 2)
    assert _hip_current_device() == before
    sc.close()


@pytest.mark.gpu
def test_gpu_python_routes_agree(engine, pkg):
    """render_denoised_spectral and render_denoised with device_mask=1 on virtual devices: assemble=True returns the tuple of the call without it, element by
    element; with one device under the mask the render leaves its own film resident and the assemble step is skipped."""
    a = pkg.api
    builder = pkg.scene.cornell_checker(rgba=True)
    rd = a.render_desc(32, 32, 10, 4)
    node = tuned_scene(engine, pkg, builder, 2)
    plain = engine.create_scene(builder)
    for sc in (node, plain):
        for kw in (dict(bin_albedo=True), dict(), dict(bin_albedo=True, specular_chain=4)):
            host = sc.render_denoised_spectral(rd, 8, 20, 0.05, device_mask=1, **kw)
            res = sc.render_denoised_spectral(rd, 8, 20, 0.05, device_mask=1, assemble=True, **kw)
            for x, y in zip(host[:5], res[:5]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), kw
        for kw in (dict(), dict(albedo=True), dict(albedo=True, specular_chain=4)):
            host = sc.render_denoised(rd, 20, 0.05, device_mask=1, **kw)
            res = sc.render_denoised(rd, 20, 0.05, device_mask=1, assemble=True, **kw)
            for x, y in zip(host[:3], res[:3]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), kw
    with pytest.raises(a.PtError, match="assemble=True needs a device_mask"):
        node.render_denoised_spectral(rd, 8, 20, 0.05, assemble=True)
    node.close(); plain.close()


@pytest.mark.gpu
def test_gpu_ptcli_denoise_assemble(pkg, tmp_path):
    """ptcli --denoise --denoise-spectral-bins 8 --demodulate-bins --develop cie --spectral-devices 1 under PT_AMD_MULTI_VIRTUAL=4 writes with
    --denoise-assemble, byte for byte, every file of the run without it."""
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    flags = ["--denoise", "--denoise-spectral-bins", "8", "--demodulate-bins", "--develop", "cie", "--spectral-devices", "1"]
    files = ["beauty.exr", "beauty.png", "beauty_denoised.exr", "beauty_denoised.png", "beauty_denoised_developed.exr", "beauty_denoised_developed.png",
             "beauty_denoised_spectral.exr", "beauty_developed.exr", "beauty_developed.png", "beauty_spectral.exr"]
    for name, extra in (("host", []), ("assembled", ["--denoise-assemble"])):
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / name)] + flags + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=dict(os.environ, PT_AMD_MULTI_VIRTUAL="4"))
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(str(tmp_path / name))) == files
    for f in files:
        assert (tmp_path / "host" / f).read_bytes() == (tmp_path / "assembled" / f).read_bytes(), f


def _hip_set_device(d):
    hip = C.CDLL("libamdhip64.so")   # (the process's HIP runtime, already loaded by the engine)
    assert hip.hipSetDevice(C.c_int(d)) == 0


@pytest.mark.gpu
def test_gpu_two_physical_devices(engine, pkg):
    """Mask 3 over two real devices (runs only where the box has them), the scene on device 0 and then on device 1: there film, counts and stats take the
    peer route too, and the shard of device 0 the staged one without being asked."""
    if engine.lib.pt_device_count() < 2:
        pytest.skip("one HIP device on this box")
    builder, rd, rel = node_desc(engine, pkg)
    before = _hip_current_device()
    for device in (0, 1):
        _hip_set_device(device)
        try:
            sc = engine.create_scene(builder)
        finally:
            _hip_set_device(before)
        film, counts, stats, spectral, _ = sc.render_adaptive_spectral_multi(rd, BINS, 40, rel, step=10, stats=True, device_mask=0b11)
        for staged in (False, True):
            sc.resident_assemble(staged=staged)
            assert_assembled(sc, (film, counts, stats, spectral), (device, staged))
        assert _hip_current_device() == before
        sc.close()
