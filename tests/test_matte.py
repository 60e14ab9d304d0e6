"""ID mattes (include/pt_denoise.h pt_render_mattes / pt_matte_extract / pt_write_exr_cryptomatte).  The definition is exact, so every
check is bit for bit: the CPU tier compares the host emulation (csrc/pt_matte_rules.h compiled for the host) with a restatement in plain Python over the probes
(camera_samples, intersect), and the writer with an EXR parser of the test's own; the GPU tier compares the engine with the emulation."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import emulation
from util import PT_ERR_INVALID_ARGUMENT, ptcli

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
SKY, NONE = 0xFFFFFFFE, 0xFFFFFFFF
# pt_write_exr / pt_write_exr_spectral of film_rgb() below, written by the commit before the writer learned string attributes
PARENT_EXR_SHA256 = {0: "72d3a2cf7fcda871b363f963e8dd1a08a9c5cfe0da6765861620278b4bfa3c4d", 2: "a5b3aedf1b0a654967249362e21404e9ea2558aba3b0a9075bd1683e5ef440ba"}
PARENT_SPECTRAL_EXR_SHA256 = "bc7958a2c2d05386524573f9e1839cdfc2dbcefd59e4b1daf0cac95dcf613eca"


@pytest.fixture(scope="session")
def emu_mt(pkg):
    """The host emulation (ptemu.cpp) with the mattes (ptemu_matte.cpp) beside it: a library of its own."""
    return emulation.load(pkg, "matte")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the restatement
def np_sample_keys(sc, rd, S, key):
    """[S, n] uint32: the key of every (sample, pixel), from the probes."""
    n = rd.width * rd.height
    px = np.arange(n, dtype=np.uint32)
    out = np.zeros((S, n), np.uint32)
    for k in range(S):
        o, d, _ = sc.camera_samples(rd, px, np.full(n, k, np.uint32))
        h = sc.intersect(o, d)
        out[k] = np.where(h["valid"] != 0, h["instance"] if key == "instance" else h["material"], np.uint32(SKY))
    return out


def py_fold_pixel(sample_keys, R):
    """The fold of one pixel in plain Python: ([(key, count)] in slot order, overflow)."""
    slots, overflow = [], 0
    for key in sample_keys:
        for s in slots:
            if s[0] == key:
                s[1] += 1
                break
        else:
            if len(slots) < R:
                slots.append([key, 1])
            else:
                overflow += 1
    return slots, overflow


def py_mattes(sample_keys, w, h, R):
    """(keys [R,H,W], coverage [R,H,W], overflow [H,W], distinct keys per pixel [H,W]) from the keys of every (sample, pixel)."""
    S, n = sample_keys.shape
    keys, cov, over, distinct = np.full((R, n), NONE, np.uint32), np.zeros((R, n), F), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for p in range(n):
        mine = [int(x) for x in sample_keys[:, p]]
        slots, overflow = py_fold_pixel(mine, R)
        assert sum(c for _, c in slots) + overflow == S   # the invariant
        for r, (key, count) in enumerate(sorted(slots, key=lambda s: (-s[1], s[0]))):
            keys[r, p] = key
            cov[r, p] = F(count) / F(S)
        over[p] = overflow
        distinct[p] = len(set(mine))
    return keys.reshape(R, h, w), cov.reshape(R, h, w), over.reshape(h, w), distinct.reshape(h, w)


def np_extract(keys, cov, selections):
    R, h, w = keys.shape
    out = np.zeros((len(selections), h, w), F)
    for m, sel in enumerate(selections):
        members = np.array(sorted(set(int(x) for x in sel) - {NONE}), dtype=np.uint32)
        acc = np.zeros((h, w), F)
        for r in range(R):
            acc = np.where(np.isin(keys[r], members), acc + cov[r], acc).astype(F)
        out[m] = acc
    return out


def py_murmur3(data, seed=0):
    """MurmurHash3_x86_32, restated."""
    M = 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M
    h, n = seed, len(data)
    for i in range(0, n - n % 4, 4):
        k = int.from_bytes(data[i:i + 4], "little")
        k = (k * 0xcc9e2d51) & M
        k = rotl(k, 15)
        k = (k * 0x1b873593) & M
        h ^= k
        h = rotl(h, 13)
        h = (h * 5 + 0xe6546b64) & M
    tail = data[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        k = (k * 0xcc9e2d51) & M
        k = rotl(k, 15)
        k = (k * 0x1b873593) & M
        h ^= k
    h ^= n
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M
    h ^= h >> 16
    return h


def py_id_bits(h):
    return h ^ (1 << 23) if ((h >> 23) & 255) in (0, 255) else h


_KEEP = []     # every emulation scene a matte was rendered on: the emulation keeps a scene's resident matte by the handle's address
_FRAMES = {}


def frame(pkg, emu, name, w, h, S, key, seed=1):
    """One emulation scene, its render desc and the keys of every (sample, pixel) per (scene, size, S, key kind): shared among the tests, never changed."""
    k = (name, w, h, S, key, seed)
    if k not in _FRAMES:
        sc = emu.create_scene(getattr(pkg.scene, name)())
        _KEEP.append(sc)
        rd = pkg.api.render_desc(w, h, 10, 4, seed=seed)
        _FRAMES[k] = (sc, rd, np_sample_keys(sc, rd, S, key))
    return _FRAMES[k]


def selection_cases(keys):
    """The selections of the extract tests for a matte's keys: (one set, sixteen sets).  The sixteen hold an empty set, the sky alone, a key that occurs
    nowhere, duplicates in no order, and the union of all keys and the sky."""
    present = [int(x) for x in np.unique(keys) if int(x) != NONE]
    objects = [k for k in present if k != SKY]
    absent = next(k for k in range(100000, 100100) if k not in present)
    union = objects + [SKY]
    sixteen = [[], [SKY], [absent], [objects[0]] * 3 + [absent, objects[0]], list(reversed(union)) + union[:2], union, [objects[-1], SKY, objects[0]], [NONE]]
    sixteen += [[k] for k in (objects * 8)[:8]]
    assert len(sixteen) == 16
    return [[objects[0]]], sixteen, union


# ------------------------------------------------------------------------------------------------ CPU tier
def test_libraries_export_the_matte_entries(pkg, emu_mt):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ("render_mattes", "mattes_resident", "matte_extract", "matte_extract_resident", "cryptomatte_hash"):
        assert hasattr(lib, "pt_" + name) and hasattr(emu_mt.lib, "ptemu_" + name), name
    assert hasattr(lib, "pt_write_exr_cryptomatte") and hasattr(emu_mt.lib, "ptemu_matte_finish_pixel")
    text = open(os.path.join(ROOT, "include", "pt_denoise.h")).read()
    assert "#define PT_MATTE_SKY  0xFFFFFFFEu" in text and "#define PT_MATTE_NONE 0xFFFFFFFFu" in text and "#define PT_MATTE_RANKS_MAX 8" in text
    assert "pt_render_mattes" not in open(os.path.join(ROOT, "include", "pt_api.h")).read()
    a = pkg.api
    assert C.sizeof(a.MatteDesc) == 16 and (a.MATTE_SKY, a.MATTE_NONE, a.MATTE_RANKS_MAX) == (SKY, NONE, 8)
    assert all(a.ENTRIES[n].channel == "denoise_last_error" for n in ("render_mattes", "mattes_resident", "matte_extract", "matte_extract_resident"))


@pytest.mark.parametrize("name,w,h,S,R,key", [("mixed_small", 40, 27, 5, 6, "instance"), ("mixed_small", 40, 27, 5, 6, "material"), ("cornell_gem", 24, 16, 4, 3, "instance")])
def test_emulated_mattes_equal_the_restatement(emu_mt, pkg, name, w, h, S, R, key):
    """R is at least the number of distinct keys of every pixel: the ranks are the exact histogram."""
    sc, rd, sample_keys = frame(pkg, emu_mt, name, w, h, S, key)
    wkeys, wcov, wover, distinct = py_mattes(sample_keys, w, h, R)
    assert int(wover.max()) == 0 and int(distinct.max()) <= R, "a pixel overflows at R = %d (%d distinct keys)" % (R, int(distinct.max()))
    keys, cov, over = sc.render_mattes(rd, S, key=key, ranks=R)
    assert keys.shape == (R, h, w) and keys.dtype == np.uint32 and cov.dtype == F and over.shape == (h, w)
    assert bits_equal(keys, wkeys) and bits_equal(cov, wcov) and bits_equal(over, wover)
    # the frame holds what it was chosen for: edges (pixels with two keys and more), sky or walls, and a rank nobody fills
    assert int(distinct.max()) >= 2 and (keys[0] != NONE).all() and (keys[R - 1] == NONE).any()
    counts = np.rint(cov.astype(np.float64) * S).astype(np.int64)
    assert np.array_equal(counts.sum(0), np.full((h, w), S))
    assert sc.mattes_resident() == (w, h, R, S)


@pytest.mark.parametrize("R", [1, 2])
def test_emulated_mattes_overflow_as_the_restatement_does(emu_mt, pkg, R):
    sc, rd, sample_keys = frame(pkg, emu_mt, "mixed_small", 40, 27, 5, "instance")
    wkeys, wcov, wover, distinct = py_mattes(sample_keys, 40, 27, R)
    assert int((wover > 0).sum()) >= 1, "no pixel of this frame overflows at R = %d" % R
    assert np.array_equal(wover > 0, distinct > R)   # (a pixel overflows exactly when it sees more keys than it has ranks)
    keys, cov, over = sc.render_mattes(rd, 5, key="instance", ranks=R)
    assert bits_equal(keys, wkeys) and bits_equal(cov, wcov) and bits_equal(over, wover)
    counts = np.rint(cov.astype(np.float64) * 5).astype(np.int64)
    assert np.array_equal(counts.sum(0) + over, np.full((27, 40), 5))


def finish_pixel(emu, slot_keys, slot_counts, samples):
    R = len(slot_keys)
    fn = emu.lib.ptemu_matte_finish_pixel
    fn.restype, fn.argtypes = C.c_int32, [C.c_uint32, u32p, u32p, C.c_uint32, u32p, f32p]
    sk, sn = np.asarray(slot_keys, np.uint32), np.asarray(slot_counts, np.uint32)
    keys, cov = np.zeros(R, np.uint32), np.zeros(R, F)
    assert fn(R, sk.ctypes.data_as(u32p), sn.ctypes.data_as(u32p), samples, keys.ctypes.data_as(u32p), cov.ctypes.data_as(f32p)) == 0
    return [int(k) for k in keys], cov


def test_finish_orders_ties_by_key_and_the_sky_by_its_value(emu_mt):
    keys, cov = finish_pixel(emu_mt, [9, SKY, 3, 7, 5, 0, 0, 0], [2, 2, 2, 4, 1, 0, 0, 0], 11)
    assert keys == [7, 3, 9, SKY, 5, NONE, NONE, NONE]
    assert bits_equal(cov, np.array([F(4) / F(11), F(2) / F(11), F(2) / F(11), F(2) / F(11), F(1) / F(11), 0, 0, 0], F))
    # an empty slot's key is ignored, whatever it holds; every R has a form of its own
    for R in range(1, 9):
        slot_keys = [40 - r for r in range(R)]
        keys, cov = finish_pixel(emu_mt, slot_keys, [1] * (R - 1) + [0], 7)
        assert keys == sorted(slot_keys[:R - 1]) + [NONE] and cov[R - 1] == 0 and all(c == F(1) / F(7) for c in cov[:R - 1])
    # every order of eight distinct counts comes out sorted (a few hundred seeded permutations) ...
    rng = np.random.default_rng(20261020)
    for _ in range(300):
        counts = rng.permutation(8) + 1
        keys, cov = finish_pixel(emu_mt, list(range(100, 108)), list(counts), 36)
        assert keys == [100 + int(i) for i in np.argsort(-counts)]
    # ... and every pattern of two count values (the 0-1 principle: the network sorts)
    for pattern in range(256):
        counts = [2 if pattern >> r & 1 else 1 for r in range(8)]
        keys, _ = finish_pixel(emu_mt, list(range(8)), counts, 16)
        assert keys == [r for r in range(8) if counts[r] == 2] + [r for r in range(8) if counts[r] == 1]


def test_emulated_extract_equals_numpy_set_arithmetic(emu_mt, pkg):
    sc, rd, _ = frame(pkg, emu_mt, "mixed_small", 40, 27, 5, "instance")
    keys, cov, _ = sc.render_mattes(rd, 5, key="instance", ranks=6)
    one, sixteen, union = selection_cases(keys)
    for selections in (one, sixteen):
        got = emu_mt.matte_extract(keys, cov, selections)
        assert got.shape == (len(selections), 27, 40) and bits_equal(got, np_extract(keys, cov, selections))
        assert bits_equal(sc.matte_extract_resident(selections), got)
    got = emu_mt.matte_extract(keys, cov, sixteen)
    assert not got[0].any() and not got[2].any() and not got[7].any()          # the empty set, the absent key, NONE
    assert bits_equal(got[1], np_extract(keys, cov, [[SKY]])[0]) and got[1].max() == 1.0   # the sky alone
    assert bits_equal(got[3], emu_mt.matte_extract(keys, cov, one)[0])           # duplicates and an absent key beside a key
    total = np.zeros((27, 40), F)
    for r in range(6):
        total = np.where(keys[r] != NONE, total + cov[r], total).astype(F)
    assert bits_equal(got[5], total) and bits_equal(got[4], total)               # the union, in any order: the fold of the coverage in rank order
    assert emu_mt.matte_extract(keys, cov, []).shape == (0, 27, 40)


HASHES = {"": 0x00000000, "hello": 0x248bfa47, "Hello, world!": 0xc0363e43, "instance0": 0x1aff6f28, "lambertian_white": 0x0dd41c3c, "CryptoObject": 0x3ae39a58}


def test_cryptomatte_hash_vectors(emu_mt, pkg):
    engine_lib = pkg.api.Library(pkg.LIBRARY_PATH, "pt_")   # host only: no device is needed
    fn = emu_mt.lib.ptemu_matte_murmur3
    fn.restype, fn.argtypes = C.c_uint32, [C.c_char_p, C.c_size_t, C.c_uint32]
    for data, seed, want in ((b"Hello, world!", 1234, 0xfaf6cdb3), (b"", 1, 0x514e28b7), (b"\xff\xff\xff\xff", 0, 0x76293b50)):
        assert fn(data, len(data), seed) == want == py_murmur3(data, seed)
    for lib in (emu_mt, engine_lib):
        for name, want in HASHES.items():
            h, i = lib.cryptomatte_hash(name)
            assert h == want == py_murmur3(name.encode()), name
            assert int(np.array([i], F).view(np.uint32)[0]) == py_id_bits(want), name
        assert int(np.array([lib.cryptomatte_hash("")[1]], F).view(np.uint32)[0]) == 0x00800000
    # a name whose hash is a denormal, an infinity or a NaN as it stands: bit 23 is flipped, nothing else
    fixed = 0
    for i in range(100000):
        name = "n%d" % i
        h = py_murmur3(name.encode())
        if ((h >> 23) & 255) not in (0, 255):
            continue
        for lib in (emu_mt, engine_lib):
            got_h, got_id = lib.cryptomatte_hash(name)
            bits = int(np.array([got_id], F).view(np.uint32)[0])
            assert got_h == h and bits == h ^ (1 << 23) and np.isfinite(got_id) and abs(got_id) >= np.finfo(F).tiny
        fixed |= 1 if ((h >> 23) & 255) == 0 else 2
        if fixed == 3:
            break
    assert fixed == 3, "no name n<i> with exponent 0 and none with exponent 255"


# ---- the writer
def parse_exr(path):
    """An uncompressed scanline OpenEXR file with FLOAT channels: (attributes {name: (type, bytes)}, channel names in file order, {name: [H,W] uint32 bits})."""
    data = open(path, "rb").read()
    assert struct.unpack_from("<I", data, 0)[0] == 20000630
    pos, attrs = 8, {}
    cstr = lambda p: (data[p:data.index(b"\0", p)].decode(), data.index(b"\0", p) + 1)
    while data[pos] != 0:
        name, pos = cstr(pos)
        kind, pos = cstr(pos)
        size = struct.unpack_from("<I", data, pos)[0]
        attrs[name] = (kind, data[pos + 4:pos + 4 + size])
        pos += 4 + size
    pos += 1
    chlist, names, p = attrs["channels"][1], [], 0
    while chlist[p] != 0:
        end = chlist.index(b"\0", p)
        names.append(chlist[p:end].decode())
        assert struct.unpack_from("<I", chlist, end + 1)[0] == 2   # FLOAT
        p = end + 1 + 16
    assert attrs["compression"][1] == b"\0"
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    offsets = struct.unpack_from("<%dQ" % h, data, pos)
    planes = {n: np.zeros((h, w), np.uint32) for n in names}
    for y in range(h):
        yy, size = struct.unpack_from("<ii", data, offsets[y])
        assert yy == y and size == 4 * w * len(names)
        for c, n in enumerate(names):
            planes[n][y] = np.frombuffer(data, "<u4", w, offsets[y] + 8 + 4 * w * c)
    assert offsets[-1] + 8 + 4 * w * len(names) == len(data)
    return attrs, names, planes


def film_rgb():
    return (np.arange(5 * 3 * 3, dtype=F).reshape(3, 5, 3) * F(0.0625) - F(0.5)).astype(F)


def test_cryptomatte_file(pkg, tmp_path):
    lib = pkg.api.Library(pkg.LIBRARY_PATH, "pt_")
    R, h, w = 3, 3, 5
    rng = np.random.default_rng(7)
    keys = rng.choice(np.array([0, 1, 2, 77, SKY, NONE], np.uint32), (R, h, w)).astype(np.uint32)
    cov = rng.random((R, h, w)).astype(F)
    names = [(0, "instance0"), (2, 'the "left" wall'), (5, "nobody")]
    rgb = film_rgb()
    for with_rgb in (False, True):
        path = str(tmp_path / ("crypto%d.exr" % with_rgb))
        lib.write_exr_cryptomatte(path, keys, cov, "CryptoObject", names=names, linear_rgb=rgb if with_rgb else None)
        attrs, channels, planes = parse_exr(path)
        layer = ["CryptoObject%02d.%s" % (nn, c) for nn in range(2) for c in "ABGR"]
        assert channels == sorted((["B", "G", "R"] if with_rgb else []) + layer)    # byte-wise name order, as the format requires
        name_of = {0: "instance0", 2: 'the "left" wall', 1: "key1", 77: "key77"}
        ident = lambda k: 0 if k in (SKY, NONE) else py_id_bits(py_murmur3(name_of[k].encode()))
        ids = np.vectorize(ident, otypes=[np.uint32])(keys)
        for r in range(R):
            assert np.array_equal(planes["CryptoObject%02d.%s" % (r // 2, "RB"[r % 2])], ids[r]), r          # the id bit patterns
            assert np.array_equal(planes["CryptoObject%02d.%s" % (r // 2, "GA"[r % 2])], cov[r].view(np.uint32)), r
        assert not planes["CryptoObject01.B"].any() and not planes["CryptoObject01.A"].any()              # the odd rank's padding
        if with_rgb:
            for c, name in enumerate("RGB"):
                assert np.array_equal(planes[name], rgb[..., c].view(np.uint32))
        prefix = "cryptomatte/3ae39a5/"
        crypto = {k[len(prefix):]: v for k, v in attrs.items() if k.startswith("cryptomatte/")}
        assert sorted(crypto) == ["conversion", "hash", "manifest", "name"] and all(k.startswith(prefix) for k in attrs if k.startswith("cryptomatte/"))
        assert all(kind == "string" for kind, _ in crypto.values())
        assert crypto["name"][1] == b"CryptoObject" and crypto["hash"][1] == b"MurmurHash3_32" and crypto["conversion"][1] == b"uint32_to_float32"
        manifest = json.loads(crypto["manifest"][1].decode(), object_pairs_hook=list)
        assert manifest == [(n, "%08x" % py_id_bits(py_murmur3(n.encode()))) for _, n in names]
    # an even number of ranks has no padding, one rank has one
    path = str(tmp_path / "two.exr")
    lib.write_exr_cryptomatte(path, keys[:2], cov[:2], "CryptoMaterial")
    attrs, channels, planes = parse_exr(path)
    assert channels == ["CryptoMaterial00.%s" % c for c in "ABGR"] and json.loads(attrs["cryptomatte/%s/manifest" % ("%08x" % py_murmur3(b"CryptoMaterial"))[:7]][1]) == {}
    for bad in (dict(keys=keys[:0], coverage=cov[:0], layer="L"), dict(keys=keys, coverage=cov, layer="")):
        with pytest.raises(pkg.api.PtError):
            lib.write_exr_cryptomatte(str(tmp_path / "bad.exr"), **bad)


def test_the_other_exr_writers_write_what_they_wrote(pkg, tmp_path):
    lib = pkg.api.Library(pkg.LIBRARY_PATH, "pt_")
    for cs, want in PARENT_EXR_SHA256.items():
        path = str(tmp_path / ("film%d.exr" % cs))
        lib.write_exr(path, film_rgb(), cs)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == want
    path = str(tmp_path / "bins.exr")
    bins = (np.arange(2 * 3 * 5, dtype=F).reshape(2, 3, 5) * F(0.25)).astype(F)
    lib.write_exr_spectral(path, np.array([450.0, 650.0], F), bins, film_rgb())
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == PARENT_SPECTRAL_EXR_SHA256


# ---- refusals
def _matte_refusals(lib, prefix, last_error, api, scene_handle, with_scene):
    """Every refusal of include/pt_denoise.h's matte section that needs no matte to be resident.  A bad matte desc is named before the scene is looked at."""
    render = getattr(lib, prefix + "render_mattes")
    render.restype, render.argtypes = C.c_int32, [C.c_void_p, C.POINTER(api.RenderDesc), C.POINTER(api.MatteDesc), u32p, f32p, u32p]
    extract = getattr(lib, prefix + "matte_extract")
    extract.restype, extract.argtypes = C.c_int32, [C.c_uint32] * 3 + [u32p, f32p, C.c_uint32, u32p, u32p, C.c_uint32, f32p]
    rd = api.render_desc(6, 5, 10, 3)

    def refused(status, word):
        assert status == PT_ERR_INVALID_ARGUMENT, word
        assert word in last_error(), (word, last_error())

    def status(md, rd_=rd, scene=scene_handle):
        return render(scene, None if rd_ is None else C.byref(rd_), None if md is None else C.byref(md), None, None, None)

    ok = api.MatteDesc(4, 3, 0)
    for md, word in ((None, b"matte"), (api.MatteDesc(0, 3, 0), b"samples"), (api.MatteDesc(65536, 3, 0), b"samples"), (api.MatteDesc(4, 0, 0), b"ranks"),
                     (api.MatteDesc(4, 9, 0), b"ranks"), (api.MatteDesc(4, 3, 2), b"key"), (api.MatteDesc(4, 3, 1, (C.c_uint32 * 1)(5)), b"reserved")):
        refused(status(md), word)
    refused(status(ok, scene=None), b"scene")
    if with_scene:
        refused(status(ok, rd_=None), b"desc")
        refused(status(ok, rd_=api.render_desc(6, 5, 10, 3, camera_index=3)), b"camera_index")
        refused(status(ok, rd_=api.render_desc(0, 5, 10, 3)), b"width")
    # the extract: too many sets, too many keys, offsets that fall
    keys, cov, out = np.zeros((2, 5, 6), np.uint32), np.zeros((2, 5, 6), F), np.zeros((17, 5, 6), F)

    def ex(set_count, offsets, n_selected, ranks=2):
        offsets, selected = np.asarray(offsets, np.uint32), np.zeros(max(n_selected, 1), np.uint32)
        return extract(6, 5, ranks, keys.ctypes.data_as(u32p), cov.ctypes.data_as(f32p), set_count, offsets.ctypes.data_as(u32p), selected.ctypes.data_as(u32p), 0,
                       out.ctypes.data_as(f32p))
    refused(ex(17, [0] * 18, 0), b"set_count")
    refused(ex(2, [0, 600, 1025], 1025), b"selected")
    refused(ex(3, [0, 5, 4, 6], 6), b"offsets")
    refused(ex(1, [1, 2], 2), b"offsets")
    refused(ex(1, [0, 1], 1, ranks=9), b"ranks")


def test_emulation_refuses_bad_matte_arguments(emu_mt, pkg):
    err = emu_mt.lib.ptemu_denoise_last_error
    err.restype = C.c_char_p
    sc = emu_mt.create_scene(pkg.scene.cornell_box())   # (never rendered on: no matte is resident)
    _matte_refusals(emu_mt.lib, "ptemu_", err, pkg.api, sc.handle, True)
    for call in (sc.mattes_resident, lambda: sc.matte_extract_resident([[0]])):
        with pytest.raises(pkg.api.PtError) as e:
            call()
        assert e.value.status == PT_ERR_INVALID_ARGUMENT and "no resident matte" in str(e.value)
    with pytest.raises(pkg.api.PtError) as e:
        sc.render_mattes(pkg.api.render_desc(6, 5, 10, 3), 4, ranks=9)
    assert "ranks" in str(e.value)
    with pytest.raises(pkg.api.PtError) as e:
        emu_mt.matte_extract(np.zeros((2, 5, 6), np.uint32), np.zeros((2, 5, 6), F), [[1]] * 17)
    assert "set_count" in str(e.value)


def test_engine_refuses_bad_matte_arguments_before_it_looks_for_a_device(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    lib.pt_last_error.restype = C.c_char_p
    _matte_refusals(lib, "pt_", lib.pt_last_error, pkg.api, None, False)
    for fn, args in ((lib.pt_mattes_resident, (None,) * 5), (lib.pt_matte_extract_resident, (None, 0, None, None, None))):
        fn.restype = C.c_int32
        assert fn(*args) == PT_ERR_INVALID_ARGUMENT and b"scene" in lib.pt_last_error()


def test_ptcli_refuses_mattes_over_a_device_mask(pkg, tmp_path):
    exe = ptcli(pkg)
    for args, words in ((["--mattes", "instance", "--devices", "3"], ("--mattes", "--devices")),
                        (["--mattes", "material", "--spectral-bins", "4", "--spectral-devices", "1"], ("--mattes", "--spectral-devices")),
                        (["--mattes", "instance", "--light-groups", "instance", "--light-group-devices", "1"], ("--mattes", "--light-group-devices")),
                        (["--mattes", "object"], ("--mattes", "instance")), (["--matte-ranks", "4"], ("--matte-ranks", "--mattes")),
                        (["--mattes", "instance", "--matte-ranks", "9"], ("--matte-ranks", "1..8")), (["--mattes", "instance", "--matte-samples", "0"], ("--matte-samples",))):
        r = subprocess.run([exe, "--output-dir", str(tmp_path / "refused")] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert r.returncode == 2 and all(wd in r.stderr for wd in words), r.stderr
    assert not (tmp_path / "refused").exists()


def test_scene_file_names_a_material_id(pkg):
    sf = pkg.scene_file
    config = sf.Config(os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c1.toml"))
    scene = sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config)
    for name in ("lambertian_white", "lambertian_red", "lambertian_green"):
        assert scene.material(name) >= 0 and scene.material_name(scene.material(name)) == name
    assert scene.material_name(pkg.api.material_id(pkg.api.TAG_MATERIAL, 0xFFFF)) is None


# ------------------------------------------------------------------------------------------------ GPU tier
def gpu_pair(engine, emu, pkg, name, w, h, S, R, key, seed=1):
    """The engine's matte against the emulation's, bit for bit; returns the engine's scene and matte."""
    esc, rd, _ = frame(pkg, emu, name, w, h, S, key, seed)
    want = esc.render_mattes(rd, S, key=key, ranks=R)
    gsc = engine.create_scene(getattr(pkg.scene, name)())
    got = gsc.render_mattes(rd, S, key=key, ranks=R)
    for g, wv, what in zip(got, want, ("keys", "coverage", "overflow")):
        assert bits_equal(g, wv), "%s: %d values differ" % (what, int((g.view(np.uint32) != wv.view(np.uint32)).sum()))
    assert gsc.mattes_resident() == (w, h, R, S)
    return gsc, esc, rd, got


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["instance", "material"])
@pytest.mark.parametrize("R", [1, 2, 6, 8])
def test_gpu_mattes_equal_the_emulation(engine, emu_mt, pkg, R, key):
    """40 x 27 = 1080 pixels: five blocks of 256 lanes, the last one ragged and its last wave ragged."""
    _, _, _, (keys, cov, over) = gpu_pair(engine, emu_mt, pkg, "mixed_small", 40, 27, 5, R, key)
    if key == "instance":   # (what the CPU tier's restatement shows for this frame)
        assert (over > 0).any() == (R < 3)
    counts = np.rint(cov.astype(np.float64) * 5).astype(np.int64)
    assert np.array_equal(counts.sum(0) + over, np.full((27, 40), 5))


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,S,R", [("test_bokeh_small", 32, 24, 6, 8), ("cornell_gem", 24, 16, 4, 3)])
def test_gpu_mattes_equal_the_emulation_on_other_scenes(engine, emu_mt, pkg, name, w, h, S, R):
    """test_bokeh_small: 82 instances behind a wide aperture, through the top-level walk."""
    _, _, _, (keys, cov, over) = gpu_pair(engine, emu_mt, pkg, name, w, h, S, R, "instance")
    assert len(np.unique(keys[keys < SKY])) >= 2


@pytest.mark.gpu
def test_gpu_mattes_twice_on_one_scene_and_a_render_between(engine, emu_mt, pkg):
    builder = pkg.scene.mixed_small()
    big, small = pkg.api.render_desc(48, 32, 2, 3, seed=3), pkg.api.render_desc(24, 16, 2, 3, seed=3)
    film_rd = pkg.api.render_desc(24, 16, 2, 3, seed=5)
    sc = engine.create_scene(builder)
    first = sc.render_mattes(big, 4, key="instance", ranks=6)
    assert sc.mattes_resident() == (48, 32, 6, 4)
    film, _ = sc.render(film_rd)
    assert sc.mattes_resident() == (48, 32, 6, 4)          # a film render leaves the matte where it is ...
    sel = [[int(first[0][0, 0, 0])], [SKY]]
    assert bits_equal(sc.matte_extract_resident(sel), engine.matte_extract(first[0], first[1], sel))
    second = sc.render_mattes(small, 3, key="material", ranks=2)
    assert sc.mattes_resident() == (24, 16, 2, 3)
    fresh = engine.create_scene(builder)
    plain_film, _ = fresh.render(film_rd)
    assert bits_equal(film, plain_film)                    # ... and a matte render leaves the film what it is
    want = fresh.render_mattes(small, 3, key="material", ranks=2)
    for g, wv in zip(second, want):
        assert bits_equal(g, wv)
    sel = [[int(k) for k in np.unique(second[0]) if int(k) != NONE]]
    assert bits_equal(sc.matte_extract_resident(sel), fresh.matte_extract_resident(sel))


@pytest.mark.gpu
def test_gpu_extract_equals_the_emulation(engine, emu_mt, pkg):
    gsc, esc, rd, (keys, cov, _) = gpu_pair(engine, emu_mt, pkg, "mixed_small", 40, 27, 5, 6, "instance")
    one, sixteen, _ = selection_cases(keys)
    for selections in (one, sixteen):
        want = emu_mt.matte_extract(keys, cov, selections)
        assert bits_equal(engine.matte_extract(keys, cov, selections), want)
        assert bits_equal(gsc.matte_extract_resident(selections), want)
    assert gsc.render_mattes(rd, 5, key="instance", ranks=6, read=False) is None   # nothing read back: the ranks are on the device
    assert bits_equal(gsc.matte_extract_resident(sixteen), engine.matte_extract(keys, cov, sixteen))
    # every R has an extract kernel of its own
    for R in (1, 3, 8):
        k, c, _ = esc.render_mattes(rd, 5, key="instance", ranks=R)
        assert bits_equal(engine.matte_extract(k, c, sixteen), emu_mt.matte_extract(k, c, sixteen)), R


@pytest.mark.gpu
def test_gpu_resident_entries_are_refused_before_a_matte_render(engine, pkg):
    sc = engine.create_scene(pkg.scene.cornell_box())
    for call in (sc.mattes_resident, lambda: sc.matte_extract_resident([[0]])):
        with pytest.raises(pkg.api.PtError) as e:
            call()
        assert e.value.status == PT_ERR_INVALID_ARGUMENT and "no resident matte" in str(e.value)
    with pytest.raises(pkg.api.PtError) as e:
        sc.render_mattes(pkg.api.render_desc(6, 5, 10, 3, camera_index=3), 4)
    assert "camera_index" in str(e.value)


@pytest.mark.gpu
def test_gpu_rank_zero_of_a_sky_pixel_is_the_sky(engine, pkg):
    """A pixel whose guide says that all S samples missed (normal sum 0, no distance) has the sky in rank 0 with coverage 1."""
    sc = engine.create_scene(pkg.scene.mixed_small())
    rd = pkg.api.render_desc(40, 27, 10, 4, seed=1)
    keys, cov, over = sc.render_mattes(rd, 5, key="instance", ranks=6)
    guides = sc.render_guides(rd, 5)
    sky = (guides == 0).all(-1)
    assert 20 <= int(sky.sum()) < sky.size
    assert (keys[0][sky] == SKY).all() and (cov[0][sky] == 1.0).all() and (keys[1][sky] == NONE).all()
    assert not ((keys[0] == SKY) & (cov[0] == 1.0))[~sky].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,layer", [("instance", "CryptoObject"), ("material", "CryptoMaterial")])
def test_gpu_ptcli_mattes(engine, pkg, tmp_path, kind, layer):
    """ptcli --mattes writes <name>_crypto.exr with the API's ranks under the names of the scene file; every other file is byte for byte what a run without
    the flag writes."""
    exe = ptcli(pkg)
    text = open(os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c1.toml")).read()
    text = text.replace("min_samples = 16", "min_samples = 10").replace("width = 256", "width = 40").replace("height = 256", "height = 27")
    assert "min_samples = 10" in text and "width = 40" in text and "height = 27" in text
    cfg = tmp_path / "config.toml"
    cfg.write_text(text)
    runs = {}
    for tag, extra in (("plain", []), ("mattes", ["--mattes", kind, "--matte-ranks", "3", "--matte-samples", "4"])):
        out = tmp_path / tag
        r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(out), "--write-film", "--seed", "5"] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = out
    plain = sorted(os.listdir(runs["plain"]))
    assert sorted(os.listdir(runs["mattes"])) == sorted(plain + ["beauty_crypto.exr"]) and len(plain) == 3
    for f in plain:
        assert open(runs["plain"] / f, "rb").read() == open(runs["mattes"] / f, "rb").read(), f
    sf = pkg.scene_file
    config = sf.Config(str(cfg))
    scene_file = sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config)
    sc = engine.create_scene(scene_file)
    keys, cov, _ = sc.render_mattes(config.render_desc(0, seed=5), 4, key=kind, ranks=3)
    attrs, channels, planes = parse_exr(str(runs["mattes"] / "beauty_crypto.exr"))
    assert channels == sorted(["B", "G", "R"] + ["%s%02d.%s" % (layer, nn, c) for nn in range(2) for c in "ABGR"])
    name_of = (lambda k: "instance%d" % k) if kind == "instance" else scene_file.material_name
    ident = lambda k: 0 if k in (SKY, NONE) else py_id_bits(py_murmur3(name_of(int(k)).encode()))
    ids = np.vectorize(ident, otypes=[np.uint32])(keys)
    for r in range(3):
        assert np.array_equal(planes["%s%02d.%s" % (layer, r // 2, "RB"[r % 2])], ids[r]), r
        assert np.array_equal(planes["%s%02d.%s" % (layer, r // 2, "GA"[r % 2])], cov[r].view(np.uint32)), r
    manifest = json.loads(attrs["cryptomatte/%s/manifest" % ("%08x" % py_murmur3(layer.encode()))[:7]][1].decode())
    present = sorted(set(int(k) for k in np.unique(keys)) - {SKY, NONE})
    assert manifest == {name_of(k): "%08x" % ident(k) for k in present} and len(manifest) >= 3
