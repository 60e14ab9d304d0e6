"""The wavelength-binned film (include/pt_spectral.h).  Everything here is bit-exact: the CPU tier compares the rules the kernel
compiles (csrc/pt_spectral_rules.h, through tests/host_emulation/ptemu_spectral.cpp) with numpy restatements and reads the spectral EXR back with a
reader of its own; the GPU tier checks that the XYZ film is pt_render's, that a one-sample range holds the sample's addends in the bins of its
wavelengths, that a longer range is their f32 fold in sample order whatever the passes, and the command line."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
from test_emulation import emu  # noqa: F401  (fixture: libptemu.so, for ptemu_xyz_bar)
from util import PT_ERR_INVALID_ARGUMENT, PT_OK, bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
F = np.float32


def fptr(a):
    return a.ctypes.data_as(f32p)


@pytest.fixture(scope="session")
def emu_sp(pkg):
    """The rules of the spectral film on the host (tests/host_emulation/ptemu_spectral.cpp beside the engine's pt_plan.cpp): a library of its own."""
    L = C.CDLL(emulation.library_path("spectral"))
    a = pkg.api
    L.ptemu_spectral_last_error.restype = C.c_char_p
    L.ptemu_spectral_bins.restype = C.c_int32
    L.ptemu_spectral_bins.argtypes = [C.c_size_t, C.c_float, C.c_float, C.c_uint32, f32p, u32p]
    L.ptemu_spectral_fold.restype = C.c_int32
    L.ptemu_spectral_fold.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, u32p, C.c_uint32, f32p]
    L.ptemu_spectral_check_args.restype = C.c_int32
    L.ptemu_spectral_check_args.argtypes = [C.c_void_p, C.POINTER(a.RenderDesc), C.POINTER(a.SpectralDesc), C.c_void_p, C.c_void_p]
    return L


# ------------------------------------------------------------------------------------------------ numpy restatement of the definition
def np_bins(lo, hi, B, lam):
    """x = (lambda - lo) / (span / (float)B); b = x < 0 ? 0 : min((uint32_t)x, B - 1); NaN -> 0.  All f32."""
    lam = np.asarray(lam, F)
    with np.errstate(all="ignore"):
        span = F(hi) - F(lo)
        x = (lam - F(lo)) / (span / F(B))
        inside = (x >= 0) & (x < F(B))
        b = np.where(inside, x, 0).astype(np.uint32)   # (the conversion truncates, and only ever sees [0, B))
        return np.where(x >= F(B), np.uint32(B - 1), b).astype(np.uint32)


def np_hero_lambdas(lo, hi, u, nl):
    """hero_lambdas (csrc/pt_stages.h) in f32: lambda_0 = lo + u * span, lambda_k = lo + frac(u + k * 0.25) * span."""
    u = np.asarray(u, F)
    span = F(hi) - F(lo)
    out = [F(lo) + u * span]
    for k in range(1, nl):
        x = u + F(k) * F(0.25)
        x = x - np.floor(x)
        out.append(F(lo) + x * span)
    return np.stack(out)


def np_fold(nl, B, lo, hi, energy, u, pixels, plane, spectral, normalize_by=None):
    """spectral [B, plane] += the samples energy [nl, S, P], wavelength samples u [S, P] of the P pixels `pixels`, in sample order; then the division."""
    S = energy.shape[1]
    for s in range(S):
        lam = np_hero_lambdas(lo, hi, u[s], nl)
        for k in range(nl):
            b = np_bins(lo, hi, B, lam[k])
            add = energy[k, s] if nl == 1 else energy[k, s] / F(4.0)
            with np.errstate(all="ignore"):
                spectral[b, pixels] = spectral[b, pixels] + add   # (one add per pixel: the pixels are distinct)
    if normalize_by is not None:
        with np.errstate(all="ignore"):
            spectral[:, pixels] = spectral[:, pixels] / F(normalize_by)
    return spectral


def emu_fold(L, nl, B, lo, hi, planes, stride, chunk, first, count, spp, range_end, normalize, pixels, plane, spectral):
    pixels = np.ascontiguousarray(pixels, np.uint32)
    st = L.ptemu_spectral_fold(nl, B, lo, hi, fptr(planes), stride, chunk, first, count, spp, range_end, normalize, pixels.ctypes.data_as(u32p), plane, fptr(spectral))
    assert st == PT_OK, L.ptemu_spectral_last_error()


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_the_spectral_entries_and_the_desc_mirrors_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ("pt_render_spectral", "pt_spectral_bin_centres", "pt_write_exr_spectral"):
        assert hasattr(lib, name), name
    assert not any("spectral" in f for f in pkg.api.API_FUNCTIONS)   # (pt_api.h's list: the boundary the oracle shares)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pt_spectral.h")).read(), flags=re.S)
    body = re.search(r"typedef struct pt_spectral_desc \{(.*?)\} pt_spectral_desc;", text, re.S).group(1)
    fields = re.findall(r"(uint32_t)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [n for _, n, _ in fields] == ["bins", "reserved"]
    want = [(n, C.c_uint32 * int(k) if k else C.c_uint32) for _, n, k in fields]
    got = list(pkg.api.SpectralDesc._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert all(C.sizeof(g[1]) == C.sizeof(w[1]) for g, w in zip(got, want))
    assert int(re.search(r"#define PT_SPECTRAL_MAX_BINS (\d+)", text).group(1)) == 64
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "pt_spectral.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(pt_spectral_desc)' + \
        "".join(", offsetof(pt_spectral_desc, %s)" % n for _, n, _ in fields) + "); return 0; }"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    A = pkg.api.SpectralDesc
    assert out == [C.sizeof(A)] + [getattr(A, n).offset for _, n, _ in fields]


@pytest.mark.parametrize("bounds", [(380.0, 750.0), (400.0, 700.0)])
@pytest.mark.parametrize("B", [1, 2, 5, 7, 8, 64])
def test_bin_rule_equals_the_numpy_restatement(emu_sp, bounds, B):
    """spectral_bin against numpy, bit for bit: the bounds and their neighbours, every bin edge and its neighbours, values outside, NaN, 10 000 draws;
    and the bin is monotone in the wavelength."""
    lo, hi = F(bounds[0]), F(bounds[1])
    inf = F(np.inf)
    lam = [lo, hi, np.nextafter(lo, -inf), np.nextafter(lo, inf), np.nextafter(hi, -inf), np.nextafter(hi, inf)]
    w = (hi - lo) / F(B)
    for b in range(B + 1):
        edge = lo + F(b) * w
        lam += [edge, np.nextafter(edge, -inf), np.nextafter(edge, inf)]
    lam += [lo - F(25.0), hi + F(25.0), F(-1e30), F(1e30), inf, -inf, F(np.nan)]
    draws = np.sort(np.random.default_rng(B * 1000 + int(lo)).uniform(float(lo), float(hi), 10000).astype(F))
    lam = np.ascontiguousarray(np.concatenate([np.array(lam, F), draws]))
    got = np.full(lam.size, 99, np.uint32)
    assert emu_sp.ptemu_spectral_bins(lam.size, lo, hi, B, fptr(lam), got.ctypes.data_as(u32p)) == PT_OK
    want = np_bins(lo, hi, B, lam)
    assert np.array_equal(got, want)
    assert got.max() <= B - 1
    assert got[0] == 0 and got[1] == B - 1 and got[2] == 0 and got[5] == B - 1      # lo, hi, just below lo, just above hi
    assert got[np.isnan(lam)].tolist() == [0]
    d = got[-10000:]
    assert np.all(np.diff(d.astype(np.int64)) >= 0) and d[0] == 0 and d[-1] == B - 1
    if B > 1:
        assert len(np.unique(d)) == B


@pytest.mark.parametrize("nl", [1, 4])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_fold_equals_the_numpy_restatement(emu_sp, nl, B):
    """ptemu_spectral_fold over synthetic planes in the engine's layout: 37 pixels, a pass of 3 samples and a second pass of 2 that continues the same
    buffer (spp 5, the division at the end of the second only), energies with 0, negative values, inf and one NaN.  Equal to numpy bit for bit, equal
    to one pass of 5 samples, and the NaN stays in its pixel's bin."""
    rng = np.random.default_rng(nl * 100 + B)
    lo, hi, P, spp, stride, plane = 380.0, 750.0, 37, 5, 64 * 3, 50
    pixels = rng.permutation(plane)[:P].astype(np.uint32)
    e = rng.exponential(1.0, (nl, spp, P)).astype(F)
    e[rng.random(e.shape) < 0.2] = 0.0
    e[rng.random(e.shape) < 0.1] *= F(-1.0)
    e[0, 1, 3] = np.inf
    e[nl - 1, 4, 7] = -0.0
    e[0, 2, 11] = np.nan
    u = rng.random((spp, P), dtype=F)
    u[0, 0], u[1, 0] = 0.0, np.nextafter(F(1.0), F(0.0))

    def planes(first, count):
        """nl + 1 planes of `stride` floats, slot = s_local * P + p (poisoned where the pass does not reach)"""
        buf = np.full((nl + 1, stride), 12345.0, F)
        for k in range(nl):
            buf[k, :count * P] = e[k, first:first + count].ravel()
        buf[nl, :count * P] = u[first:first + count].ravel()
        return buf

    two = np.zeros((B, plane), F)
    emu_fold(emu_sp, nl, B, lo, hi, planes(0, 3), stride, P, 0, 3, spp, spp, 1, pixels, plane, two)
    mid = np_fold(nl, B, lo, hi, e[:, :3], u[:3], pixels, plane, np.zeros((B, plane), F))
    assert np.array_equal(bits(two), bits(mid))                     # (no division yet: the first pass does not reach range_end)
    emu_fold(emu_sp, nl, B, lo, hi, planes(3, 2), stride, P, 3, 2, spp, spp, 1, pixels, plane, two)
    want = np_fold(nl, B, lo, hi, e, u, pixels, plane, np.zeros((B, plane), F), normalize_by=spp)
    assert np.array_equal(bits(two), bits(want))
    one = np.zeros((B, plane), F)
    emu_fold(emu_sp, nl, B, lo, hi, planes(0, 5), stride, P, 0, 5, spp, spp, 1, pixels, plane, one)
    assert np.array_equal(bits(one), bits(two))
    # a partial range (normalize 0) leaves the running sum
    part = np.zeros((B, plane), F)
    emu_fold(emu_sp, nl, B, lo, hi, planes(0, 5), stride, P, 0, 5, spp, spp, 0, pixels, plane, part)
    assert np.array_equal(bits(part), bits(np_fold(nl, B, lo, hi, e, u, pixels, plane, np.zeros((B, plane), F))))
    # the NaN: in the bin of its wavelength, in its pixel, and nowhere else; pixels outside the list untouched
    nan_at = np.argwhere(np.isnan(two))
    nan_bin = int(np_bins(lo, hi, B, np_hero_lambdas(lo, hi, u[2, 11], nl)[0]))
    inf_bin = int(np_bins(lo, hi, B, np_hero_lambdas(lo, hi, u[1, 3], nl)[0]))
    assert nan_at.tolist() == [[nan_bin, int(pixels[11])]], nan_at
    assert two[inf_bin, pixels[3]] == np.inf
    rest = np.setdiff1d(np.arange(plane), pixels)
    assert np.all(bits(two[:, rest]) == 0)


def test_validation_rejects_each_rule_with_its_own_message(emu_sp, pkg):
    a = pkg.api
    rd = a.render_desc(8, 8, 10, 3)
    buf = np.zeros(4, F)
    ptr = buf.ctypes.data
    msgs = {}

    def status(key, scene=ptr, rdp=rd, sd=None, film=ptr, spectral=ptr):
        sd = a.SpectralDesc(5) if sd is None else sd
        st = emu_sp.ptemu_spectral_check_args(scene, C.byref(rdp) if rdp is not None else None, C.byref(sd) if sd != "null" else None, film, spectral)
        if st != PT_OK:
            msgs[key] = emu_sp.ptemu_spectral_last_error().decode()
        return st

    assert status("ok") == PT_OK
    assert status("ok1", sd=a.SpectralDesc(1)) == PT_OK and status("ok64", sd=a.SpectralDesc(64)) == PT_OK
    assert status("medium", rdp=a.render_desc(8, 8, 10, 3, medium_aware=True)) == PT_OK      # allowed: one wavelength, nothing differs
    assert status("zero", sd=a.SpectralDesc(0)) == PT_ERR_INVALID_ARGUMENT
    assert status("many", sd=a.SpectralDesc(65)) == PT_ERR_INVALID_ARGUMENT
    for k in range(3):
        sd = a.SpectralDesc(5)
        sd.reserved[k] = 1
        assert status("reserved", sd=sd) == PT_ERR_INVALID_ARGUMENT
    assert status("scene", scene=None) == PT_ERR_INVALID_ARGUMENT
    assert status("rd", rdp=None) == PT_ERR_INVALID_ARGUMENT
    assert status("sd", sd="null") == PT_ERR_INVALID_ARGUMENT
    assert status("film", film=None) == PT_ERR_INVALID_ARGUMENT
    assert status("spectral", spectral=None) == PT_ERR_INVALID_ARGUMENT
    assert set(msgs) == {"zero", "many", "reserved", "scene", "rd", "sd", "film", "spectral"}
    assert all(msgs.values()) and len(set(msgs.values())) == len(msgs), msgs
    assert "bins" in msgs["zero"] and "64" in msgs["many"] and "reserved" in msgs["reserved"]


def read_exr(path):
    """A small reader of what pt_write_exr_spectral writes: magic, version, attributes, chlist, the offset table, uncompressed scanlines of FLOAT channels."""
    data = open(path, "rb").read()
    magic, version = struct.unpack_from("<II", data, 0)
    assert magic == 20000630 and version & 0xff == 2 and not version & 0x200      # (scanline file)
    pos, attrs = 8, {}

    def cstr(p):
        e = data.index(b"\0", p)
        return data[p:e].decode(), e + 1
    while data[pos] != 0:
        name, pos = cstr(pos)
        kind, pos = cstr(pos)
        size, = struct.unpack_from("<I", data, pos)
        attrs[name] = (kind, data[pos + 4:pos + 4 + size])
        pos += 4 + size
    pos += 1
    assert attrs["compression"] == ("compression", b"\0") and attrs["lineOrder"] == ("lineOrder", b"\0")
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    kind, ch = attrs["channels"]
    assert kind == "chlist"
    names, p = [], 0
    while ch[p] != 0:
        e = ch.index(b"\0", p)
        name = ch[p:e].decode()
        ptype, plinear, xs, ys = struct.unpack_from("<iB3xii", ch, e + 1)
        assert ptype == 2 and xs == 1 and ys == 1
        assert len(name) <= 31 or version & 0x400
        names.append(name)
        p = e + 1 + 16
    assert p == len(ch) - 1
    offsets = struct.unpack_from("<%dQ" % h, data, pos)
    assert offsets[0] == pos + 8 * h
    planes = np.zeros((len(names), h, w), F)
    for y in range(h):
        yy, size = struct.unpack_from("<ii", data, offsets[y])
        assert yy == y0 + y and size == 4 * w * len(names)
        planes[:, y, :] = np.frombuffer(data, "<f4", w * len(names), offsets[y] + 8).reshape(len(names), w)
    assert offsets[-1] + 8 + 4 * w * len(names) == len(data)
    return names, planes, attrs


def channel_name(centre):
    return ("S0.%.6fnm" % float(centre)).replace(".", ",").replace("S0,", "S0.", 1)


def check_spectral_exr(path, centres, spectral, rgb):
    names, planes, attrs = read_exr(path)
    want = {channel_name(c): spectral[b] for b, c in enumerate(centres)}
    if rgb is not None:
        want.update({"R": rgb[..., 0], "G": rgb[..., 1], "B": rgb[..., 2]})
    assert names == sorted(want, key=lambda s: s.encode())                        # byte-wise name order, as the format requires
    assert attrs["spectralLayoutVersion"] == ("string", b"1.0") and attrs["emissiveUnits"] == ("string", b"W.m^-2.sr^-1")
    for name, plane in zip(names, planes):
        assert np.array_equal(bits(plane), bits(want[name])), name


def test_spectral_exr_round_trip(pkg, tmp_path):
    """pt_write_exr_spectral is host code: the library loads without a device (as in test_abi.py) and a 5x3 file of 3 bins, with and without RGB, is read
    back by the reader above — channel names and their order, the two attributes, every float."""
    lib = pkg.load()
    rng = np.random.default_rng(2)
    spectral = rng.normal(0.0, 1.0, (3, 3, 5)).astype(F)
    spectral[1, 2, 4], spectral[0, 0, 0] = np.inf, -0.0
    rgb = rng.random((3, 5, 3), dtype=F)
    centres = lib.spectral_bin_centres(pkg.api.render_desc(5, 3, 1, 1, wavelength=(380.0, 750.0)), 3)
    w = (F(750.0) - F(380.0)) / F(3)
    assert np.array_equal(bits(centres), bits(np.array([F(380.0) + (F(b) + F(0.5)) * w for b in range(3)], F)))
    assert channel_name(F(565.0)) == "S0.565,000000nm"
    for with_rgb in (True, False):
        path = str(tmp_path / ("s%d.exr" % with_rgb))
        lib.write_exr_spectral(path, centres, spectral, rgb if with_rgb else None)
        check_spectral_exr(path, centres, spectral, rgb if with_rgb else None)
    # centres whose names do not sort in numeric order (95 nm after 565 nm, byte-wise) and the refusals
    odd = np.array([95.0, 565.0, 1050.5], F)
    path = str(tmp_path / "odd.exr")
    lib.write_exr_spectral(path, odd, spectral, rgb)
    check_spectral_exr(path, odd, spectral, rgb)
    assert read_exr(path)[0] == ["B", "G", "R", "S0.1050,500000nm", "S0.565,000000nm", "S0.95,000000nm"]
    with pytest.raises(pkg.api.PtError, match="share"):
        lib.write_exr_spectral(path, np.array([500.0, 500.0, 600.0], F), spectral)
    with pytest.raises(pkg.api.PtError, match="finite"):
        lib.write_exr_spectral(path, np.array([500.0, np.nan, 600.0], F), spectral)
    # the RGB writer shares the scanline writer: its file is the spectral file's R, G, B
    lib.write_exr(str(tmp_path / "rgb.exr"), rgb)
    names, planes, attrs = read_exr(str(tmp_path / "rgb.exr"))
    assert names == ["B", "G", "R"] and "spectralLayoutVersion" not in attrs and np.array_equal(planes[2], rgb[..., 0])


# ------------------------------------------------------------------------------------------------ GPU tier
W, H, SPP, BOUNCES, B16 = 16, 12, 20, 4, 16
BOUNDS = (380.0, 750.0)
CASES = {
    "cornell": ("cornell_box", dict()),                            # the lean / fused form
    "gem": ("cornell_gem", dict()),                                # parked
    "hdri": ("hdri_small", dict()),                                # FULL
    "cornell_hero": ("cornell_box", dict(hero_wavelengths=4)),
    "fog_medium": ("fog_ball", dict(medium_aware=True)),
}
_cache = {}


def wavelength_samples(sc, pkg, w, h, seed, samples):
    """The wavelength sample u of every (sample, pixel): pt_camera_samples over the bounds (0, 1) returns 0 + u * 1 = u."""
    rd01 = pkg.api.render_desc(w, h, SPP, BOUNCES, seed=seed, wavelength=(0.0, 1.0))
    px = np.tile(np.arange(w * h, dtype=np.uint32), samples)
    ss = np.repeat(np.arange(samples, dtype=np.uint32), w * h)
    return sc.camera_samples(rd01, px, ss)[2].reshape(samples, w * h)


def case(engine, pkg, name):
    """Per scene, rendered once and shared: pt_render's film, the 20 one-sample spectral renders at 16 bins, the wavelengths, the 20-sample renders."""
    if name not in _cache:
        make, kw = CASES[name]
        a = pkg.api
        sc = engine.create_scene(getattr(pkg.scene, make)())
        rd = a.render_desc(W, H, SPP, BOUNCES, seed=7, wavelength=BOUNDS, **kw)
        c = {"sc": sc, "rd": rd, "nl": kw.get("hero_wavelengths", 1), "kw": kw}
        c["render"] = sc.render(rd)
        c["full"] = {B: sc.render_spectral(rd, B) for B in (16, 1, 5, 64)}
        c["ones"] = [sc.render_spectral(a.render_desc(W, H, SPP, BOUNCES, seed=7, wavelength=BOUNDS, first_sample=s, sample_count=1, **kw), B16) for s in range(SPP)]
        c["u"] = wavelength_samples(sc, pkg, W, H, 7, SPP)
        lam0 = sc.camera_samples(rd, np.tile(np.arange(W * H, dtype=np.uint32), SPP), np.repeat(np.arange(SPP, dtype=np.uint32), W * H))[2].reshape(SPP, W * H)
        c["lam"] = np_hero_lambdas(BOUNDS[0], BOUNDS[1], c["u"], c["nl"])          # [nl, S, P]
        assert np.array_equal(bits(c["lam"][0]), bits(lam0))                       # (the restatement is the engine's wavelength)
        _cache[name] = c
    return _cache[name]


def xyz_bar(emu, lam_nm):
    fn = emu.lib.ptemu_xyz_bar
    fn.restype = None
    fn.argtypes = [C.c_size_t, f32p, C.c_int, f32p]
    ang = np.ascontiguousarray(np.asarray(lam_nm, F) * F(10.0))
    out = np.zeros((ang.size, 3), F)
    fn(ang.size, fptr(ang), 0, fptr(out))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_the_film_is_untouched(engine, pkg, name):
    """render_spectral's XYZ film is render's byte for byte, and the ray counters are equal: one scene per kernel family."""
    c = case(engine, pkg, name)
    film, prof = c["render"]
    for B, (sfilm, spectral, sprof) in c["full"].items():
        assert film.tobytes() == sfilm.tobytes(), B
        assert (prof.camera_rays, prof.bounce_rays, prof.shadow_rays, prof.light_rays, prof.env_hits) == \
            (sprof.camera_rays, sprof.bounce_rays, sprof.shadow_rays, sprof.light_rays, sprof.env_hits)
        assert spectral.shape == (B, H, W) and np.all(np.isfinite(spectral))
    assert np.any(c["full"][16][1] != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_one_sample_exactly(engine, emu, pkg, name):
    """A one-sample range holds the sample's addends: the only non-zero bins of a pixel are the bins of its wavelengths, and the energies read from
    them, times the colour-matching functions, are the one-sample XYZ film bit for bit (in stage_accumulate_pixel's order for hero wavelengths)."""
    c = case(engine, pkg, name)
    nl, P = c["nl"], W * H
    excluded = total = 0
    zero = F(0.0)
    for s in range(SPP):
        film, spectral, _ = c["ones"][s]
        S = spectral.reshape(B16, P)
        xyz = film.reshape(P, 4)
        lam = c["lam"][:, s]                                                        # [nl, P]
        b = np.stack([np_bins(BOUNDS[0], BOUNDS[1], B16, lam[k]) for k in range(nl)])
        if nl == 4:   # at least span / 4 apart: with 16 bins the four never share one
            assert all(np.all(b[i] != b[j]) for i in range(4) for j in range(i))
        own = np.zeros((B16, P), bool)
        own[b, np.arange(P)[None, :]] = True
        assert np.all(bits(S)[~own] == 0)                                           # every other bin is +0
        addend = S[b, np.arange(P)[None, :]]                                        # [nl, P]: S = 0.0f + addend
        xb = np.stack([xyz_bar(emu, lam[k]) for k in range(nl)])                     # [nl, P, 3]
        with np.errstate(all="ignore"):
            if nl == 1:
                e = addend[0]
                assert np.all(bits(S.sum(0))[e == 0] == 0)                          # a pixel without energy: all bins +0
                t = zero + e[:, None] * xb[0]
                ok = np.ones(P, bool)
            else:
                e = addend * F(4.0)                                                 # e_k / 4.0f is exact unless it is subnormal
                ok = ~np.any((addend != 0) & (np.abs(addend) < np.finfo(F).tiny), axis=0)
                cc = zero + e[0][:, None] * xb[0]
                for k in range(1, 4):
                    cc = cc + e[k][:, None] * xb[k]
                t = zero + cc / F(4.0)
            want = zero + t                                                         # (the phase flush: f += t)
        excluded += int((~ok).sum())
        total += P
        assert np.array_equal(bits(xyz[ok, :3]), bits(want[ok])), s
        assert np.all(bits(xyz[:, 3]) == 0)
    assert excluded * 100 < total, (excluded, total)


def rebinned(c, B):
    """The definition in numpy over the recovered per-sample addends: [B, P] after SPP samples, divided by (float)SPP."""
    nl, P = c["nl"], W * H
    S = np.zeros((B, P), F)
    cols = np.arange(P)
    for s in range(SPP):
        one = c["ones"][s][1].reshape(B16, P)
        for k in range(nl):
            lam = c["lam"][k, s]
            add = one[np_bins(BOUNDS[0], BOUNDS[1], B16, lam), cols]                 # the sample's addend (e, or e_k / 4.0f) as the 16-bin render holds it
            b = np_bins(BOUNDS[0], BOUNDS[1], B, lam)
            S[b, cols] = S[b, cols] + add
    return S / F(SPP)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_the_sum_is_the_f32_fold_in_sample_order(engine, pkg, name):
    """The 20-sample spectral film is the f32 fold of the twenty one-sample films in sample order, divided by 20.0f: at 16 bins from the films themselves,
    at 1, 5 and 64 bins from the per-sample addends re-binned in numpy (at 1 bin the four hero addends of a sample meet in one bin, in k order)."""
    c = case(engine, pkg, name)
    S = np.zeros((B16, H, W), F)
    for s in range(SPP):
        S = S + c["ones"][s][1]
    assert np.array_equal(bits(c["full"][16][1]), bits(S / F(SPP)))
    for B in (16, 1, 5, 64):
        assert np.array_equal(bits(c["full"][B][1].reshape(B, W * H)), bits(rebinned(c, B))), B


@pytest.mark.gpu
def test_gpu_independent_of_passes_and_forms(engine, pkg):
    """batch_slots 1024 cuts the 3840 samples into several passes, some of which continue a pixel; with it and each of PT_TUNE_NO_LDS, PT_TUNE_NO_FUSE and
    PT_TUNE_GENERAL_FORMS the bins (and the film) are the default's."""
    a = pkg.api
    builder = pkg.scene.cornell_box()
    rd = a.render_desc(W, H, SPP, BOUNCES, seed=7, wavelength=BOUNDS)
    ref = engine.create_scene(builder).render_spectral(rd, 7)
    assert np.any(ref[1] != 0)
    for flags in (0, a.TUNE_NO_LDS, a.TUNE_NO_FUSE, a.TUNE_GENERAL_FORMS):
        t = engine.tuning_default()
        t.batch_slots = 1024
        t.flags |= flags
        got = engine.create_scene(builder, tuning=t).render_spectral(rd, 7)
        assert got[2].kernel_launches[0] > ref[2].kernel_launches[0]                # (more generate launches: more passes)
        assert np.array_equal(bits(got[1]), bits(ref[1])), flags
        assert got[0].tobytes() == ref[0].tobytes(), flags


@pytest.mark.gpu
def test_gpu_shards_are_disjoint_and_sum_to_the_film(engine, pkg):
    """40x9 with 8x8 tiles (ragged right and bottom) over three shards: outside its shard a spectral film is 0, and the three add up — zeros to values — to
    the unsharded one."""
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_box())
    kw = dict(seed=7, wavelength=BOUNDS, tile=(8, 8))
    whole = sc.render_spectral(a.render_desc(40, 9, SPP, BOUNCES, **kw), 7)
    parts = [sc.render_spectral(a.render_desc(40, 9, SPP, BOUNCES, shard=(i, 3), **kw), 7) for i in range(3)]
    owned = [np.any(p[0] != 0, axis=-1) | np.any(p[1] != 0, axis=0) for p in parts]
    assert np.all(owned[0].astype(int) + owned[1] + owned[2] <= 1)
    assert all(o.any() for o in owned)
    for p, o in zip(parts, owned):
        assert np.all(bits(p[1])[:, ~o] == 0)
    assert np.array_equal(parts[0][1] + parts[1][1] + parts[2][1], whole[1])
    assert np.array_equal(parts[0][0] + parts[1][0] + parts[2][0], whole[0])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 1)])
def test_gpu_awkward_sizes_equal_the_emulations_fold(engine, emu_sp, pkg, w, h):
    """One pixel, and one lane more than a workgroup: the 20-sample film at 7 bins equals ptemu_spectral_fold over the energies of the one-sample films."""
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_box())
    P = w * h
    kw = dict(seed=9, wavelength=BOUNDS)
    full = sc.render_spectral(a.render_desc(w, h, SPP, BOUNCES, **kw), 7)[1]
    planes = np.zeros((2, SPP * P), F)
    for s in range(SPP):
        one = sc.render_spectral(a.render_desc(w, h, SPP, BOUNCES, first_sample=s, sample_count=1, **kw), B16)[1].reshape(B16, P)
        assert np.all((one != 0).sum(0) <= 1)
        planes[0, s * P:(s + 1) * P] = one.sum(0)                                   # (one non-zero bin: the sum is the energy)
    rd01 = a.render_desc(w, h, SPP, BOUNCES, seed=9, wavelength=(0.0, 1.0))
    planes[1] = sc.camera_samples(rd01, np.tile(np.arange(P, dtype=np.uint32), SPP), np.repeat(np.arange(SPP, dtype=np.uint32), P))[2]
    want = np.zeros((7, P), F)
    emu_fold(emu_sp, 1, 7, BOUNDS[0], BOUNDS[1], planes, SPP * P, P, 0, SPP, SPP, SPP, 1, np.arange(P), P, want)
    assert np.any(want != 0)
    assert np.array_equal(bits(full.reshape(7, P)), bits(want))


def scaled_c2_config(pkg):
    """data/config_cornell_c2.toml at 32x32 and 20 spp, with a premultiply so that the factor of the EXR payload is not 1."""
    text = open(os.path.join(pkg.PACKAGE_DIR, "data", "config_cornell_c2.toml")).read()
    text, n1 = re.subn(r"min_samples = \d+", "min_samples = 20", text)
    text, n2 = re.subn(r"width = \d+\nheight = \d+", "width = 32\nheight = 32", text)
    text, n3 = re.subn(r"only_direct = false\n", "only_direct = false\npremultiply = 2.0\n", text)
    assert (n1, n2, n3) == (1, 1, 1)
    return text


@pytest.mark.gpu
def test_gpu_ptcli_spectral_bins(engine, pkg, tmp_path):
    """ptcli --spectral-bins 8: <name>_spectral.exr holds render_spectral's bins times the factor beside the payload's R, G, B; the usual PNG and EXR are
    byte for byte those of a run without the flag; the refused combinations exit non-zero with their message."""
    sf = pkg.scene_file
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    plain, spec = run("plain"), run("spec", "--spectral-bins", "8")
    assert plain.returncode == 0 and spec.returncode == 0, plain.stdout + plain.stderr + spec.stdout + spec.stderr
    assert "beauty_spectral.exr (8 bins)" in spec.stdout
    assert not (tmp_path / "plain" / "beauty_spectral.exr").exists()
    for ext in ("png", "exr"):
        assert (tmp_path / "plain" / ("beauty." + ext)).read_bytes() == (tmp_path / "spec" / ("beauty." + ext)).read_bytes(), ext
    config = sf.Config(str(cfg))
    rd, od = config.render_desc(0, seed=1), config.output_desc(0)
    assert (rd.width, rd.height, rd.spp) == (32, 32, 20) and od.factor == 2.0
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    film, spectral, _ = sc.render_spectral(rd, 8)
    _, linear = engine.output_film(film, od.tonemap, od.luminance_only, od.exposure, od.key_value, od.white_point, od.colorspace, od.factor)
    check_spectral_exr(str(tmp_path / "spec" / "beauty_spectral.exr"), engine.spectral_bin_centres(rd, 8), spectral * F(od.factor), linear)
    for extra, word in ((["--adaptive", "0.05"], "--adaptive"), (["--denoise"], "--denoise"), (["--devices", "3"], "--devices")):
        r = run("refused", "--spectral-bins", "8", *extra)
        assert r.returncode != 0 and "--spectral-bins cannot be combined with " + word in r.stderr, r.stderr
        assert not (tmp_path / "refused" / "beauty.exr").exists()
    for bad in ("0", "65", "x"):
        r = run("refused", "--spectral-bins", bad)
        assert r.returncode != 0 and "--spectral-bins needs a count in 1..64" in r.stderr
    assert "--spectral-bins" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
