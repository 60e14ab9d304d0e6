"""The resident set and the filter that runs on it (include/pt_resident.h, DESIGN.md section 14, "The resident filter").  The contract is exact: every
output of pt_denoise_resident is bit for bit the host-array entry's for the same arrays, so every comparison here is bit for bit.  The CPU tier compares
the quad route — csrc/pt_denoise_resident_rules.h compiled for the host, tests/host_emulation/ptemu_denoise_resident.cpp — with the existing emulation of
pt_denoise_spectral_albedo and the index rule with a numpy restatement, and checks every refusal; the GPU tier compares the engine's resident entries with
its host-array entries on synthetic and rendered inputs, walks the life of the resident set, and compares the command line's files."""
import ctypes as C
import filecmp
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
import test_denoise_spectral as ts
import test_denoise_spectral_albedo as tba
from test_denoise import bits_equal, np_variance
from test_spectral import scaled_c2_config
from util import PT_ERR_INVALID_ARGUMENT, PT_ERR_NO_DEVICE, PT_OK

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
u32p, f64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_float)
ENTRIES = ("pt_resident_info", "pt_resident_guides", "pt_resident_load", "pt_denoise_resident", "pt_spectral_project_resident_denoised")
# the (B mod 8, B mod 4) remainder chain of the plane-major gather against the (Q mod 2) chain of the quad gather, pads 0..3, and the cap
CPU_BINS = (1, 3, 4, 5, 7, 8, 9, 12, 13, 64)
COMBOS = ((True, True), (True, False), (False, True), (False, False))   # (XYZ albedo, per-bin albedo)


@pytest.fixture(scope="session")
def emu_res(pkg):
    """The host emulation with every filter, the guide passes, the projection and the resident entries beside them: a library of its own."""
    L = emulation.load(pkg, "denoise_resident")
    L.lib.ptemu_bins_to_quads.argtypes = [C.c_uint32, C.c_uint32, f32p, f32p]
    L.lib.ptemu_quads_to_bins.argtypes = [C.c_uint32, C.c_uint32, f32p, f32p]
    L.lib.ptemu_quad_count.restype = C.c_uint32
    L.lib.ptemu_quad_count.argtypes = [C.c_uint32]
    L.lib.ptemu_resident_end.argtypes = [C.c_void_p]
    return L


# ------------------------------------------------------------------------------------------------ inputs
_CASES = {}


def resident_case(w, h, seed, B):
    """test_denoise_spectral_albedo.synthetic_case (sky, pixels dead through the film or the statistics, one through an infinite bin, one through the bins'
    division) with, where the film leaves live pixels for them, one more pixel dead through a NaN bin alone and one through an infinite film channel alone.
    (inputs, spectral, albedo, bin_albedo), computed once per case and never written."""
    key = (w, h, seed, B)
    if key not in _CASES:
        inputs, spectral, albedo, bin_albedo, taken = tba.synthetic_case(w, h, seed, B)
        film, counts, stats, guides = (a.copy() for a in inputs)
        spectral = spectral.copy()
        live = np.isfinite(film[..., :3]).all(-1) & np.isfinite(np_variance(counts, stats)) & np.isfinite(spectral).all(0)
        free = [(int(y), int(x)) for y, x in zip(*np.nonzero(live)) if (int(y), int(x)) not in taken]
        if len(free) >= 4:   # (keep live pixels on the small films)
            spectral[0, free[0][0], free[0][1]] = np.nan
            film[free[-1][0], free[-1][1], 2] = np.inf
        for a in (film, counts, stats, guides, spectral, albedo, bin_albedo):
            a.setflags(write=False)
        _CASES[key] = ((film, counts, stats, guides), spectral, albedo, bin_albedo)
    return _CASES[key]


def host_call(lib, inputs, spectral, albedo, bin_albedo, **kw):
    """(film, variance, bins or None) from the host-array entry the arrays select"""
    if spectral is None:
        out, var = lib.denoise_film(*inputs, variance=True, albedo=albedo, **kw)
        return out, var, None
    if albedo is None and bin_albedo is None and lib.prefix == "pt_":
        out, sp, var = lib.denoise_spectral(*inputs, spectral, variance=True, **kw)
    else:
        out, sp, var = lib.denoise_spectral_albedo(*inputs, spectral, albedo, bin_albedo, variance=True, **kw)
    return out, var, sp


def resident_call(sc, spectral=True, **kw):
    """(film, variance, bins or None) from the resident entry"""
    res = sc.denoise_resident(film=True, variance=True, spectral=spectral, **kw)
    return (res[0], res[1], res[2]) if spectral else (res[0], res[1], None)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("film", "variance", "bins")):
        if w is None:
            assert g is None, (what, name)
            continue
        assert bits_equal(g, w), (what, "%s: %d values differ" % (name, int((np.ascontiguousarray(g, F).view(np.uint32) != np.ascontiguousarray(w, F).view(np.uint32)).sum())))


def fresh(lib, pkg):
    """a scene with nothing resident"""
    return lib.create_scene(pkg.scene.cornell_box())


# ------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("B", CPU_BINS)
@pytest.mark.parametrize("w,h,seed", ts.SIZES)
def test_quad_route_equals_the_plane_major_emulation(emu_res, pkg, w, h, seed, B):
    """to-quads, the passes with dn_gather_pixel_bins4, to-bins against the existing emulation of pt_denoise_spectral_albedo: film, variance and every bin,
    with both albedos, each alone and neither; the planar flag gives the same again.  The three kinds of dead pixel come out as they went in."""
    inputs, spectral, albedo, bin_albedo = resident_case(w, h, seed, B)
    sc = fresh(emu_res, pkg)
    for has_a, has_b in COMBOS:
        a, b = (albedo if has_a else None), (bin_albedo if has_b else None)
        emu_res.lib.ptemu_resident_end(sc.handle)
        sc.resident_load(*inputs, spectral=spectral, albedo=a, bin_albedo=b)
        dead = tba.np_dead(inputs[0], inputs[1], inputs[2], spectral, a, b)
        for kw in ts.params_for(w, h):
            want = host_call(emu_res, inputs, spectral, a, b, **kw)
            got = resident_call(sc, **kw)
            assert_same(got, want, (has_a, has_b, kw, "quads"))
            assert_same(resident_call(sc, planar=True, **kw), want, (has_a, has_b, kw, "planar"))
            assert bits_equal(got[2][:, dead], spectral[:, dead]) and bits_equal(got[0][dead][:, :3], inputs[0][dead][:, :3])
            assert np.all(np.isfinite(got[2][:, ~dead]))
    sc.close()


@pytest.mark.parametrize("chain", (0, 4))
def test_resident_guides_keep_what_the_guide_entries_return(emu_res, pkg, chain):
    """resident_guides on the emulation: the filter over the guides, the albedo and the per-bin albedo it kept equals the host-array emulation over what
    render_guides_bin_albedo (render_guides without the albedos) returns for the same desc; the parts not asked for are resident no longer."""
    a = pkg.api
    inputs, spectral, _, _ = resident_case(9, 7, 21, 5)
    sc = emu_res.create_scene(pkg.scene.cornell_checker(rgba=True))
    rd = a.render_desc(9, 7, 10, 4)
    sc.resident_load(*inputs[:3], spectral=spectral)
    sc.resident_guides(rd, 2, specular_chain=chain, albedo=True, bin_albedo=True)
    assert sc.resident_info() == (9, 7, 5, a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES | a.RESIDENT_ALBEDO | a.RESIDENT_BIN_ALBEDO)
    guides, alb, balb = sc.render_guides_bin_albedo(rd, 5, 2, chain)
    assert_same(resident_call(sc), host_call(emu_res, inputs[:3] + (guides,), spectral, alb, balb), "both albedos")
    sc.resident_guides(rd, 2, specular_chain=chain)
    assert sc.resident_info()[3] == a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES
    assert_same(resident_call(sc), host_call(emu_res, inputs[:3] + (guides,), spectral, None, None), "guides alone")
    sc.close()


def test_the_cases_hold_the_three_kinds_of_dead_pixel():
    """A NaN bin, an infinite film channel and a bin that the division alone makes infinite, each on a pixel that is live otherwise."""
    inputs, spectral, albedo, bin_albedo = resident_case(64, 40, 11, 9)
    film, counts, stats, _ = inputs
    fine_film = np.isfinite(film[..., :3]).all(-1) & np.isfinite(np_variance(counts, stats))
    assert (np.isnan(spectral).any(0) & fine_film).any()
    assert (np.isinf(film[..., :3]).any(-1) & np.isfinite(spectral).all(0)).any()
    with np.errstate(all="ignore"):
        q = spectral / np.maximum(bin_albedo, F(1e-3))
    assert (np.isinf(q).any(0) & np.isfinite(spectral).all(0) & fine_film).any()


@pytest.mark.parametrize("B", CPU_BINS)
def test_index_rule_equals_its_numpy_restatement(emu_res, B):
    """Quad q of pixel p holds bins 4q .. 4q+3 at element q * plane + p; the pads hold 0.0f; the round trip is the identity on the real bins."""
    n = 37
    rng = np.random.default_rng(B)
    planes = rng.standard_normal((B, n)).astype(F)
    Q = (B + 3) // 4
    assert emu_res.lib.ptemu_quad_count(B) == Q
    quads = np.full((Q, n, 4), 7.0, F)
    emu_res.lib.ptemu_bins_to_quads(n, B, planes.ctypes.data_as(f32p), quads.ctypes.data_as(f32p))
    want = np.zeros((4 * Q, n), F)
    want[:B] = planes
    want = np.ascontiguousarray(want.reshape(Q, 4, n).transpose(0, 2, 1))
    assert bits_equal(quads, want)
    assert np.all(quads.transpose(0, 2, 1).reshape(4 * Q, n)[B:].view(np.uint32) == 0)   # the pads: +0.0f
    back = np.full((B, n), 7.0, F)
    emu_res.lib.ptemu_quads_to_bins(n, B, quads.ctypes.data_as(f32p), back.ctypes.data_as(f32p))
    assert bits_equal(back, planes)


def refusals(lib, pkg, sc, other):
    """Every refusal of the five entries on `sc`, a scene with nothing resident (`other`: a second such scene): {name: message}.  Each is an invalid argument."""
    a = pkg.api
    L, p = lib.lib, lib.prefix
    got = {}

    def refused(name, fn, *args):
        st = fn(*args)
        assert st == PT_ERR_INVALID_ARGUMENT, (name, st)
        err = lib._resident_last_error
        got[name] = err().decode() if err else lib.last_error()

    inputs, spectral, albedo, bin_albedo = resident_case(5, 3, 13, 5)
    film, counts, stats, guides = inputs
    fp = lambda x: x.ctypes.data_as(f32p)
    load = lambda s, w, h, b, f=None, c=None, st=None, sp=None, g=None, al=None, ba=None: lib._resident_load(
        s, w, h, b, fp(f) if f is not None else None, c.ctypes.data_as(u32p) if c is not None else None, st.ctypes.data_as(f64p) if st is not None else None,
        fp(sp) if sp is not None else None, fp(g) if g is not None else None, fp(al) if al is not None else None, fp(ba) if ba is not None else None)
    info = a.ResidentInfo()
    rd = a.render_desc(5, 3, 10, 4)
    dd = a.ResidentDenoiseDesc()
    M = np.ones((3, 5), F)
    out = np.zeros((3, 3, 5), F)
    h = sc.handle
    # null scenes and null arguments
    refused("info_scene", lib._resident_info, None, C.byref(info))
    refused("info_null", lib._resident_info, h, None)
    refused("guides_scene", lib._resident_guides, None, C.byref(rd), 4, None, 0)
    refused("guides_desc", lib._resident_guides, h, None, 4, None, 0)
    refused("load_scene", load, None, 5, 3, 0, film, counts, stats)
    refused("denoise_scene", lib._denoise_resident, None, C.byref(dd), None, None, None)
    refused("denoise_desc", lib._denoise_resident, h, None, None, None, None)
    refused("project_scene", lib._spectral_project_resident_denoised, None, 3, fp(M), fp(out))
    refused("project_out", lib._spectral_project_resident_denoised, h, 3, fp(M), None)
    # nothing resident
    refused("guides_no_film", lib._resident_guides, h, C.byref(rd), 4, None, 0)
    refused("denoise_no_film", lib._denoise_resident, h, C.byref(dd), None, None, None)
    refused("project_no_bins", lib._spectral_project_resident_denoised, h, 3, fp(M), fp(out))
    # pt_resident_load's own
    refused("load_nothing", load, h, 5, 3, 0)
    refused("load_size", load, h, 0, 3, 0, film, counts, stats)
    refused("load_31_bits", load, h, 1 << 16, 1 << 16, 0, film, counts, stats)
    refused("load_together", load, h, 5, 3, 0, film, counts)
    refused("load_bins_0", load, h, 5, 3, 0, None, None, None, spectral)
    refused("load_bins_65", load, h, 5, 3, 65, None, None, None, spectral)
    low = counts.copy(); low[1, 1] = 1
    refused("load_count", load, h, 5, 3, 0, film, low, stats)
    bad_g = guides.copy(); bad_g[0, 0, 3] = np.nan
    refused("load_guide", load, h, 5, 3, 0, None, None, None, None, bad_g)
    bad_a = albedo.copy(); bad_a[0, 0, 1] = -1.0
    refused("load_albedo", load, h, 5, 3, 0, None, None, None, None, None, bad_a)
    bad_b = bin_albedo.copy(); bad_b[0, 0, 0] = np.inf
    refused("load_bin_albedo", load, h, 5, 3, 5, None, None, None, None, None, None, bad_b)
    assert lib._resident_info(h, C.byref(info)) == PT_OK and (info.width, info.height, info.bins, info.parts) == (0, 0, 0, 0)   # a refused load left nothing
    # with a film and bins resident, but no guides
    assert load(h, 5, 3, 5, film, counts, stats, spectral) == PT_OK
    assert lib._resident_info(h, C.byref(info)) == PT_OK and (info.width, info.height, info.bins, info.parts) == (5, 3, 5, a.RESIDENT_FILM | a.RESIDENT_BINS)
    refused("load_other_size", load, h, 3, 5, 0, None, None, None, None, guides)
    refused("load_other_bins", load, h, 5, 3, 4, None, None, None, None, None, None, bin_albedo[:4])
    refused("denoise_no_guides", lib._denoise_resident, h, C.byref(dd), None, None, None)
    refused("guides_flag", lib._resident_guides, h, C.byref(rd), 4, None, 32)
    refused("guides_bin_without_albedo", lib._resident_guides, h, C.byref(rd), 4, None, a.RESIDENT_BIN_ALBEDO)
    refused("guides_size", lib._resident_guides, h, C.byref(a.render_desc(3, 5, 10, 4)), 4, None, 0)
    refused("guides_samples", lib._resident_guides, h, C.byref(rd), 0, None, 0)
    refused("guides_chain", lib._resident_guides, h, C.byref(rd), 4, C.byref(a.GuideChainDesc(17, 0.0)), 0)
    assert load(other.handle, 5, 3, 0, film, counts, stats) == PT_OK
    refused("guides_bins", lib._resident_guides, other.handle, C.byref(rd), 4, None, a.RESIDENT_ALBEDO | a.RESIDENT_BIN_ALBEDO)
    # with guides too
    assert load(h, 5, 3, 0, None, None, None, None, guides) == PT_OK
    refused("denoise_flag", lib._denoise_resident, h, C.byref(a.ResidentDenoiseDesc(a.DenoiseDesc(), 2)), None, None, None)
    refused("denoise_reserved", lib._denoise_resident, h, C.byref(a.ResidentDenoiseDesc(a.DenoiseDesc(), 0, (C.c_uint32 * 3)(0, 0, 1))), None, None, None)
    refused("denoise_half_size", lib._denoise_resident, h, C.byref(a.ResidentDenoiseDesc(a.DenoiseDesc(5, 0))), None, None, None)
    refused("denoise_size", lib._denoise_resident, h, C.byref(a.ResidentDenoiseDesc(a.DenoiseDesc(3, 5))), None, None, None)
    refused("denoise_iterations", lib._denoise_resident, h, C.byref(a.ResidentDenoiseDesc(a.DenoiseDesc(0, 0, 11))), None, None, None)
    refused("denoise_sigma", lib._denoise_resident, h, C.byref(a.ResidentDenoiseDesc(a.DenoiseDesc(0, 0, 0, -1.0))), None, None, None)
    assert load(other.handle, 5, 3, 0, None, None, None, None, guides) == PT_OK
    refused("denoise_out_spectral", lib._denoise_resident, other.handle, C.byref(dd), None, None, fp(np.zeros((5, 3, 5), F)))
    refused("project_before_filter", lib._spectral_project_resident_denoised, h, 3, fp(M), fp(out))
    return got, (h, dd, M, out, fp)


def test_every_refusal_has_its_own_message(emu_res, pkg):
    """Each refusal of each new entry is an invalid argument with a message of its own (the emulation runs the engine's checks, pt_plan.cpp's); after a
    filter run the projection refuses a bad matrix as pt_spectral_project_resident does."""
    sc, other = fresh(emu_res, pkg), fresh(emu_res, pkg)
    got, (h, dd, M, out, fp) = refusals(emu_res, pkg, sc, other)
    # (the two "no resident film" and the two "before a filter run" cases share their entry's one message)
    same = [("denoise_no_film", "denoise_no_film"), ("project_no_bins", "project_before_filter")]
    distinct = [k for k in got if k not in ("project_before_filter",)]
    assert len({got[k] for k in distinct}) == len(distinct), got
    for x, y in same:
        assert got[x] == got[y]
    for name, word in (("info_scene", "pt_resident_info"), ("guides_no_film", "no resident film"), ("denoise_no_film", "no resident film"),
                       ("denoise_no_guides", "no resident guides"), ("project_no_bins", "no resident denoised bins"), ("load_together", "come together"),
                       ("load_count", "below 2"), ("load_guide", "guide value"), ("load_albedo", "albedo value"), ("load_bin_albedo", "bin_albedo value"),
                       ("guides_bin_without_albedo", "needs PT_RESIDENT_ALBEDO"), ("guides_bins", "needs resident bins"), ("denoise_reserved", "reserved"),
                       ("denoise_out_spectral", "out_spectral"), ("load_other_size", "stay resident"), ("guides_chain", "max_chain")):
        assert word in got[name], (name, got[name])
    assert emu_res._denoise_resident(h, C.byref(dd), None, None, None) == PT_OK
    a = pkg.api
    assert sc.resident_info()[3] == a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES | a.RESIDENT_DENOISED | a.RESIDENT_DENOISED_BINS
    for K, matrix, word in ((17, np.ones((17, 5), F), "at most 16"), (0, M, "K must be positive"), (3, None, "matrix is null")):
        st = emu_res._spectral_project_resident_denoised(h, K, fp(matrix) if matrix is not None else None, fp(out))
        assert st == PT_ERR_INVALID_ARGUMENT and word in emu_res._resident_last_error().decode()
    with pytest.raises(ValueError):
        sc.spectral_project_resident(np.ones((3, 4), F), denoised=True)
    den_bins = sc.denoise_resident(film=False, spectral=True)
    assert bits_equal(sc.spectral_project_resident(M, denoised=True), emu_res.spectral_project(den_bins, M))
    sc.close(); other.close()


def test_the_engine_refuses_before_it_looks_for_a_device(pkg):
    """The product's entries run the same checks first: with no scene — there is none to make where there is no device — each is refused as an invalid
    argument with its own message, never as PT_ERR_NO_DEVICE."""
    a = pkg.api
    lib = pkg.load()
    info, rd, dd = a.ResidentInfo(), a.render_desc(5, 3, 10, 4), a.ResidentDenoiseDesc()
    film, counts, stats = np.zeros((3, 5, 4), F), np.full((3, 5), 2, np.uint32), np.zeros((3, 5, 2))
    M, out = np.ones((3, 5), F), np.zeros((3, 3, 5), F)
    fp = lambda x: x.ctypes.data_as(f32p)
    calls = {"pt_resident_info": lambda: lib._resident_info(None, C.byref(info)),
             "pt_resident_guides": lambda: lib._resident_guides(None, C.byref(rd), 4, None, 0),
             "pt_resident_load": lambda: lib._resident_load(None, 5, 3, 0, fp(film), counts.ctypes.data_as(u32p), stats.ctypes.data_as(f64p), None, None, None, None),
             "pt_denoise_resident": lambda: lib._denoise_resident(None, C.byref(dd), None, None, None),
             "pt_spectral_project_resident_denoised": lambda: lib._spectral_project_resident_denoised(None, 3, fp(M), fp(out))}
    messages = set()
    for name in ENTRIES:
        assert calls[name]() == PT_ERR_INVALID_ARGUMENT, name
        assert name in lib.last_error() and "scene is null" in lib.last_error()
        messages.add(lib.last_error())
    assert len(messages) == len(ENTRIES)


def test_library_exports_the_entries_and_the_header_stands_alone(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    a = pkg.api
    assert not any(n.startswith("resident") or n == "denoise_resident" for n in a.API_FUNCTIONS)   # (pt_api.h's list: the boundary the oracle shares)
    text = open(os.path.join(ROOT, "include", "pt_resident.h")).read()
    assert "pt_api.h" not in re.findall(r'#include "([^"]+)"', text) and re.findall(r'#include "([^"]+)"', text) == ["pt_spectral.h"]
    src = '#include "pt_resident.h"\n#include <stdio.h>\n#include <stddef.h>\n' \
          'typedef pt_status (*filter_fn)(pt_scene*, const pt_resident_denoise_desc*, float*, float*, float*);\nfilter_fn f = pt_denoise_resident;\n' \
          'int main(void) { printf("%zu %zu %zu %zu %u %u\\n", sizeof(struct pt_resident_info), sizeof(pt_resident_denoise_desc), offsetof(pt_resident_denoise_desc, flags), ' \
          'offsetof(pt_resident_denoise_desc, reserved), PT_RESIDENT_DENOISED_BINS, PT_RESIDENT_PLANAR_GATHER); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        for ext, cc, std in ((".c", "gcc", "-std=c99"), (".cpp", "g++", "-std=c++17")):   # the header alone, as C and as C++
            open(os.path.join(d, "t" + ext), "w").write(src)
            subprocess.check_call([cc, std, "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t.o"), os.path.join(d, "t" + ext)])
        open(os.path.join(d, "s.c"), "w").write(src.replace("filter_fn f = pt_denoise_resident;\n", ""))
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "s")], text=True).split()]
    assert sizes == [C.sizeof(a.ResidentInfo), C.sizeof(a.ResidentDenoiseDesc), a.ResidentDenoiseDesc.flags.offset, a.ResidentDenoiseDesc.reserved.offset,
                     a.RESIDENT_DENOISED_BINS, a.RESIDENT_PLANAR_GATHER]


# ------------------------------------------------------------------------------------------------ GPU tier
GPU_SIZES = [(64, 40, 11), (37, 53, 12), (5, 3, 13), (1, 9, 14), (9, 1, 15), (257, 3, 16)]   # ragged 32x8 tiles, films below one tile, step-16 taps that leave the film
GPU_BINS = (1, 5, 9, 64)


@pytest.fixture(scope="module")
def holder(engine, pkg):
    """One engine scene whose resident set the synthetic tests load and reload: its kept buffers grow to the largest case and are reused by the rest."""
    sc = engine.create_scene(pkg.scene.cornell_box())
    yield sc
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", GPU_BINS)
@pytest.mark.parametrize("w,h,seed", GPU_SIZES)
def test_gpu_resident_filter_equals_the_host_array_entry_on_synthetic_inputs(engine, pkg, w, h, seed, B):
    """resident_load of the synthetic inputs, dead pixels included, then denoise_resident in its quad and its planar form against denoise_spectral(_albedo) on
    the same arrays: one pass and five, the four albedo combinations."""
    inputs, spectral, albedo, bin_albedo = resident_case(w, h, seed, B)
    for has_a, has_b in COMBOS:
        a, b = (albedo if has_a else None), (bin_albedo if has_b else None)
        sc = engine.create_scene(pkg.scene.cornell_box())   # (a scene per combination: an albedo once loaded stays resident)
        sc.resident_load(*inputs, spectral=spectral, albedo=a, bin_albedo=b)
        for iterations in (1, 5):
            want = host_call(engine, inputs, spectral, a, b, iterations=iterations)
            assert_same(resident_call(sc, iterations=iterations), want, (has_a, has_b, iterations, "quads"))
            assert_same(resident_call(sc, iterations=iterations, planar=True), want, (has_a, has_b, iterations, "planar"))
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", GPU_SIZES)
def test_gpu_resident_film_filter_equals_the_host_array_entry_on_synthetic_inputs(engine, pkg, w, h, seed):
    """Without bins the resident filter is denoise_film, with an albedo denoise_film_albedo."""
    inputs, _, albedo, _ = resident_case(w, h, seed, 5)
    for a in (None, albedo):
        sc = engine.create_scene(pkg.scene.cornell_box())
        sc.resident_load(*inputs, albedo=a)
        for iterations in (1, 5):
            assert_same(resident_call(sc, spectral=False, iterations=iterations), host_call(engine, inputs, None, a, None, iterations=iterations), (a is not None, iterations))
        sc.close()


@pytest.mark.gpu
def test_gpu_repeated_calls_reuse_the_set(engine, holder):
    """A second and a third call with other parameters on the same resident set equal those calls' host-array results: the sources are not clobbered and the
    kept buffers are reused; a smaller film loaded afterwards is filtered in the same buffers."""
    for w, h, seed, B in ((64, 40, 11, 9), (37, 53, 12, 5)):
        inputs, spectral, albedo, bin_albedo = resident_case(w, h, seed, B)
        holder.resident_load(*inputs, spectral=spectral, albedo=albedo, bin_albedo=bin_albedo)
        for kw in ({}, dict(sigma_luminance=1.5), dict(sigma_luminance=9.0, planar=True), dict(sigma_luminance=1.5)):
            host_kw = {k: v for k, v in kw.items() if k != "planar"}
            assert_same(resident_call(holder, **kw), host_call(engine, inputs, spectral, albedo, bin_albedo, **host_kw), (w, h, kw))


def rendered(engine, pkg, builder, chain):
    a = pkg.api
    sc = engine.create_scene(builder)
    rd = a.render_desc(32, 32, 10, 4)
    film, counts, stats, spectral, _ = sc.render_adaptive_spectral(rd, 8, 20, 0.05, stats=True)
    return sc, rd, (film, counts, stats), spectral


@pytest.mark.gpu
@pytest.mark.parametrize("chain", (0, 8))
def test_gpu_rendered_film_filtered_and_developed_where_it_lies(engine, pkg, chain):
    """render_adaptive_spectral, resident_guides with both albedos (at the first hit, and at the end of a specular chain of 8 through the glass slab),
    denoise_resident and both developments against the host entries called by hand on the arrays the render and render_guides_bin_albedo returned."""
    a = pkg.api
    builder = pkg.scene.cornell_checker_slab() if chain else pkg.scene.cornell_checker(rgba=True)
    sc, rd, (film, counts, stats), spectral = rendered(engine, pkg, builder, chain)
    assert sc.resident_info() == (32, 32, 8, a.RESIDENT_FILM | a.RESIDENT_BINS)
    M = engine.spectral_observer_matrix(rd, 8)
    before = sc.spectral_project_resident(M)
    sc.resident_guides(rd, 4, specular_chain=chain, albedo=True, bin_albedo=True)
    assert sc.resident_info()[3] == a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES | a.RESIDENT_ALBEDO | a.RESIDENT_BIN_ALBEDO
    guides, alb, balb = sc.render_guides_bin_albedo(rd, 8, 4, chain)   # (a guide pass of the host entry's writes nothing of the resident set)
    want = host_call(engine, (film, counts, stats, guides), spectral, alb, balb)
    assert_same(resident_call(sc), want, "quads")
    assert bits_equal(sc.spectral_project_resident(M, denoised=True), engine.spectral_project(want[2], M))
    assert_same(resident_call(sc, planar=True), want, "planar")
    assert bits_equal(sc.spectral_project_resident(M, denoised=True), engine.spectral_project(want[2], M))
    assert bits_equal(sc.spectral_project_resident(M), before) and bits_equal(before, engine.spectral_project(spectral, M))   # the undenoised bins: untouched
    assert sc.denoise_resident(film=False) is None   # nothing asked for: nothing comes back, the outputs stay resident
    assert sc.resident_info()[3] & (a.RESIDENT_DENOISED | a.RESIDENT_DENOISED_BINS) == a.RESIDENT_DENOISED | a.RESIDENT_DENOISED_BINS
    # guides alone: the joint filter without demodulation, pt_denoise_spectral
    sc.resident_guides(rd, 4, specular_chain=chain)
    assert sc.resident_info()[3] == a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES
    assert_same(resident_call(sc), host_call(engine, (film, counts, stats, guides), spectral, None, None), "no albedo")
    sc.close()


@pytest.fixture(scope="module")
def slab_film(engine, pkg):
    """One adaptive spectral render of the glass-slab scene, 33 x 17 with 4 bins, left resident on its scene and never written: 561 pixels are more than one
    256-thread block, no multiple of 64 and end in a ragged wave; the slab gives the guide samples chains of both lengths."""
    sc = engine.create_scene(pkg.scene.cornell_checker_slab())
    rd = pkg.api.render_desc(33, 17, 10, 4)
    film, counts, stats, spectral, _ = sc.render_adaptive_spectral(rd, 4, 20, 0.05, stats=True)
    for arr in (film, counts, stats, spectral):
        arr.setflags(write=False)
    yield sc, rd, (film, counts, stats), spectral
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("albedo,bin_albedo", ((False, False), (True, False), (True, True)))
@pytest.mark.parametrize("chain", (0, 3))
def test_gpu_resident_guide_pass_in_every_form_filtered_where_it_lies(engine, pkg, slab_film, chain, albedo, bin_albedo):
    """resident_guides at the first hit and with a chain of 3, with guides only, with the albedo and with both albedos (3 guide samples), then denoise_resident
    in both forms against the host-array filter over what the host-array guide entry of the same form returned."""
    a = pkg.api
    sc, rd, inputs, spectral = slab_film
    sc.resident_guides(rd, 3, specular_chain=chain, albedo=albedo, bin_albedo=bin_albedo)
    assert sc.resident_info() == (33, 17, 4, a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES | (a.RESIDENT_ALBEDO if albedo else 0) |
                                  (a.RESIDENT_BIN_ALBEDO if bin_albedo else 0))
    if bin_albedo:
        guides, alb, balb = sc.render_guides_bin_albedo(rd, 4, 3, chain)
    elif chain:
        guides, alb, balb = sc.render_guides_chain(rd, 3, chain, albedo=albedo) + (None,)
    else:
        guides, alb, balb = sc.render_guides_albedo(rd, 3) + (None,) if albedo else (sc.render_guides(rd, 3), None, None)
    want = host_call(engine, inputs + (guides,), spectral, alb, balb)
    assert_same(resident_call(sc), want, (chain, albedo, bin_albedo, "quads"))
    assert_same(resident_call(sc, planar=True), want, (chain, albedo, bin_albedo, "planar"))


@pytest.mark.gpu
def test_gpu_film_only_after_render_adaptive(engine, pkg):
    """After render_adaptive there are no bins: the resident filter is denoise_film, and with resident_guides(albedo=True) denoise_film_albedo."""
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_checker(rgba=True))
    rd = a.render_desc(32, 32, 10, 4)
    film, counts, stats, _ = sc.render_adaptive(rd, 20, 0.05, stats=True)
    assert sc.resident_info() == (32, 32, 0, a.RESIDENT_FILM)
    sc.resident_guides(rd, 4)
    guides, alb = sc.render_guides_albedo(rd, 4)
    assert_same(resident_call(sc, spectral=False), host_call(engine, (film, counts, stats, guides), None, None, None), "film")
    sc.resident_guides(rd, 4, albedo=True)
    assert_same(resident_call(sc, spectral=False), host_call(engine, (film, counts, stats, guides), None, alb, None), "film, albedo")
    with pytest.raises(a.PtError, match="out_spectral without resident bins"):
        sc.denoise_resident(spectral=True)
    with pytest.raises(a.PtError, match="no resident denoised bins"):
        sc.spectral_project_resident(np.ones((3, 8), F), denoised=True)
    sc.close()


@pytest.mark.gpu
def test_gpu_life_of_the_resident_set(engine, pkg):
    """A fresh scene, a scene after a plain render, after a node render on two virtual devices and a scene without guides are refused; a new adaptive render
    drops guides and denoised outputs; resident_load does not make pt_spectral_project_resident succeed."""
    a = pkg.api
    rd = a.render_desc(32, 32, 10, 4)
    sc = engine.create_scene(pkg.scene.cornell_checker(rgba=True))
    assert sc.resident_info() == (0, 0, 0, 0)
    with pytest.raises(a.PtError, match="pt_denoise_resident: the scene has no resident film"):
        sc.denoise_resident()
    with pytest.raises(a.PtError, match="pt_resident_guides: the scene has no resident film"):
        sc.resident_guides(rd)
    sc.render_adaptive_spectral(rd, 8, 20, 0.05, stats=True)
    with pytest.raises(a.PtError, match="no resident guides"):
        sc.denoise_resident()
    sc.resident_guides(rd, 4, albedo=True, bin_albedo=True)
    sc.denoise_resident()
    assert sc.resident_info() == (32, 32, 8, 127)
    sc.render_adaptive_spectral(rd, 8, 20, 0.05, stats=True)
    assert sc.resident_info() == (32, 32, 8, a.RESIDENT_FILM | a.RESIDENT_BINS)   # guides, albedos and denoised outputs went when the render started
    sc.render_adaptive(rd, 20, 0.05, stats=True)
    assert sc.resident_info() == (32, 32, 0, a.RESIDENT_FILM)
    sc.render(rd)
    assert sc.resident_info() == (0, 0, 0, 0)
    with pytest.raises(a.PtError, match="no resident film"):
        sc.denoise_resident()
    # resident_load is not a render: pt_spectral_project_resident stays refused on a scene that has rendered no spectral film
    loaded = engine.create_scene(pkg.scene.cornell_box())
    inputs, spectral, _, _ = resident_case(5, 3, 13, 5)
    loaded.resident_load(*inputs, spectral=spectral)
    assert loaded.resident_info() == (5, 3, 5, a.RESIDENT_FILM | a.RESIDENT_BINS | a.RESIDENT_GUIDES) and loaded.spectral_resident() is None
    with pytest.raises(a.PtError, match="no resident spectral film"):
        loaded.spectral_project_resident(np.ones((3, 5), F))
    loaded.close()
    # ... and leaves a render's resident spectral film as it is
    M = engine.spectral_observer_matrix(rd, 8)
    _, sp, _ = sc.render_spectral(rd, 8)
    want = sc.spectral_project_resident(M)
    sc.resident_load(*inputs, spectral=spectral)
    assert bits_equal(sc.spectral_project_resident(M), want) and bits_equal(want, engine.spectral_project(sp, M))
    sc.close()
    # a node render leaves packed shards, no film one device can filter
    t = engine.tuning_default()
    t.multi_virtual = 2
    node = engine.create_scene(pkg.scene.cornell_checker(rgba=True), tuning=t)
    node.render_adaptive_spectral(rd, 8, 20, 0.05, stats=True)
    assert node.resident_info()[3] == a.RESIDENT_FILM | a.RESIDENT_BINS
    node.render_adaptive_spectral_multi(rd, 8, 20, 0.05, stats=True, device_mask=1)
    assert node.resident_info() == (0, 0, 0, 0)
    with pytest.raises(a.PtError, match="no resident film"):
        node.denoise_resident()
    node.close()


@pytest.mark.gpu
def test_gpu_python_routes_agree(engine, pkg):
    """render_denoised_spectral(resident=True) and render_denoised(resident=True) return the tuples of resident=False, element by element."""
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_checker(rgba=True))
    rd = a.render_desc(32, 32, 10, 4)
    for kw in (dict(bin_albedo=True), dict(), dict(bin_albedo=True, specular_chain=4)):
        host = sc.render_denoised_spectral(rd, 8, 20, 0.05, **kw)
        res = sc.render_denoised_spectral(rd, 8, 20, 0.05, resident=True, **kw)
        for x, y in zip(host[:5], res[:5]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), kw
    for kw in (dict(), dict(albedo=True), dict(albedo=True, specular_chain=4)):
        host = sc.render_denoised(rd, 20, 0.05, **kw)
        res = sc.render_denoised(rd, 20, 0.05, resident=True, **kw)
        for x, y in zip(host[:3], res[:3]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), kw
    with pytest.raises(a.PtError, match="device_mask"):
        sc.render_denoised_spectral(rd, 8, 20, 0.05, resident=True, device_mask=1)
    sc.close()


@pytest.mark.gpu
def test_gpu_ptcli_denoise_resident(engine, pkg, tmp_path):
    """ptcli --denoise --denoise-spectral-bins 8 --demodulate-bins --develop cie --denoise-resident writes, byte for byte, the files of the run without the
    last flag; so do the film-only and the undemodulated routes; the flag is refused without --denoise and with a node render."""
    exe = os.path.join(pkg.PACKAGE_DIR, "csrc", "ptcli")
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    routes = {"full": ["--denoise", "--denoise-spectral-bins", "8", "--demodulate-bins", "--develop", "cie"],
              "plain": ["--denoise", "--denoise-spectral-bins", "8"],
              "film": ["--denoise", "--demodulate-albedo"]}
    for name, flags in routes.items():
        host, res = run(name + "_host", *flags), run(name + "_res", *flags, "--denoise-resident")
        assert host.returncode == 0 and res.returncode == 0, host.stdout + host.stderr + res.stdout + res.stderr
        files = sorted(os.listdir(tmp_path / (name + "_host")))
        assert files == sorted(os.listdir(tmp_path / (name + "_res"))) and len(files) >= 4
        for f in files:
            assert filecmp.cmp(tmp_path / (name + "_host") / f, tmp_path / (name + "_res") / f, shallow=False), (name, f)
    for extra, message in ((["--denoise-resident"], "--denoise-resident needs --denoise"),
                           (["--denoise", "--denoise-resident", "--devices", "1"], "--denoise-resident cannot be combined with --devices"),
                           (["--denoise", "--denoise-spectral-bins", "8", "--denoise-resident", "--spectral-devices", "1"],
                            "--denoise-resident cannot be combined with --spectral-devices")):
        r = run("refused", *extra)
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "refused" / "beauty.exr").exists()
    assert "--denoise-resident" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
