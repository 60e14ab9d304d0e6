"""Developing the spectral film (include/pt_spectral.h): pt_spectral_response_matrix, pt_spectral_project and its resident form.
The CPU tier compares the rules the kernel compiles (csrc/pt_spectral_project_rules.h, through tests/host_emulation/ptemu_spectral_project.cpp) and the
host-only matrix entry with numpy restatements, bit for bit, and checks every refusal; the GPU tier checks the kernel's bits, the resident film, the matrix
against the device's curve evaluator, that a film developed with the colour-matching rows is the XYZ film within a derived bound, and the command line."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import emulation
from test_emulation import emu  # noqa: F401  (fixture: libptemu.so, for ptemu_xyz_bar and the emulation's curve evaluator)
from test_spectral import scaled_c2_config
from util import PT_ERR_INVALID_ARGUMENT, PT_OK, bits, ptcli

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-pathtracer_amd", "csrc")
REF = os.path.join(HERE, "golden", "reference_tree")
u32p, i32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)
F = np.float32
BOUNDS = (380.0, 750.0)


def fptr(a):
    return a.ctypes.data_as(f32p)


@pytest.fixture(scope="session")
def emu_pj(pkg):
    """The rules of a development on the host (ptemu_spectral_project.cpp beside the engine's pt_plan.cpp and pt_scene_host.cpp): a library of its own."""
    L = C.CDLL(emulation.library_path("spectral_project"))
    a = pkg.api
    L.ptemu_spectral_project_last_error.restype = C.c_char_p
    L.ptemu_spectral_project.restype = C.c_int32
    L.ptemu_spectral_project.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptemu_spectral_check_matrix.restype = C.c_int32
    L.ptemu_spectral_check_matrix.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.ptemu_spectral_response_matrix.restype = C.c_int32
    L.ptemu_spectral_response_matrix.argtypes = [C.POINTER(a.RenderDesc), C.POINTER(a.SpectralDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
    L.ptemu_spectral_sample_lambdas.restype = C.c_int32
    L.ptemu_spectral_sample_lambdas.argtypes = [C.c_float, C.c_float, C.c_uint32, C.c_uint32, f32p]
    return L


# ------------------------------------------------------------------------------------------------ numpy restatements of the rules
def np_project(matrix, spectral):
    """out[k] = the f32 fold over b ascending of acc = acc + M[k, b] * S_b, from 0.0f; multiply and add are two f32 operations.  spectral [B, ...]."""
    matrix = np.asarray(matrix, F)
    spectral = np.asarray(spectral, F)
    K, B = matrix.shape
    out = np.zeros((K,) + spectral.shape[1:], F)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = np.zeros(spectral.shape[1:], F)
            for b in range(B):
                acc = acc + matrix[k, b] * spectral[b]
            out[k] = acc
    return out


def np_sample_lambdas(lo, hi, B, n):
    """lambda[b, j] = lo + ((float)b + ((float)j + 0.5f) / (float)n) * w, w = (hi - lo) / (float)B; all f32."""
    lo, hi = F(lo), F(hi)
    w = (hi - lo) / F(B)
    b = np.arange(B, dtype=F)[:, None]
    j = np.arange(n, dtype=F)[None, :]
    return (lo + (b + (j + F(0.5)) / F(n)) * w).astype(F)


def np_matrix_row(r, f, n):
    """r, f [B, n] per-wavelength values (f None: no filter): m = 0.0f; m = m + r * f over j ascending; m / (float)n."""
    m = np.zeros(r.shape[0], F)
    for j in range(n):
        m = m + (r[:, j] * f[:, j] if f is not None else r[:, j])
    return m / F(n)


def xyz_bar(emu, lam_nm):  # noqa: F811
    fn = emu.lib.ptemu_xyz_bar
    fn.restype = None
    fn.argtypes = [C.c_size_t, f32p, C.c_int, f32p]
    ang = np.ascontiguousarray(np.asarray(lam_nm, F).ravel() * F(10.0))
    out = np.zeros((ang.size, 3), F)
    fn(ang.size, fptr(ang), 0, fptr(out))
    return out.reshape(np.shape(lam_nm) + (3,))


def planes(rng, B, shape):
    """normal-range finite values of both signs, no zeros"""
    s = rng.uniform(0.05, 4.0, (B,) + shape).astype(F)
    s[rng.random(s.shape) < 0.4] *= F(-1.0)
    return s


def weights(rng, K, B):
    m = rng.uniform(0.01, 2.0, (K, B)).astype(F)
    m[rng.random(m.shape) < 0.3] *= F(-1.0)
    return m


# ------------------------------------------------------------------------------------------------ CPU tier
def test_library_exports_the_entries_and_the_mirrors_match_the_header(pkg):
    lib = C.CDLL(pkg.LIBRARY_PATH)
    for name in ("pt_spectral_response_matrix", "pt_spectral_project", "pt_spectral_project_resident", "pt_spectral_resident"):
        assert hasattr(lib, name), name
    assert hasattr(C.CDLL(pkg.scene_file.LIBRARY_PATH), "pt_scene_file_library_curve")
    assert not any("spectral" in f for f in pkg.api.API_FUNCTIONS)   # (pt_api.h's list: the boundary the oracle shares)
    a = pkg.api
    # a small C program: the constants, the size of pt_curve, and every entry assigned to a pointer of the type the ctypes binding assumes (a mismatch does not compile)
    src = r'''#include <stdio.h>
#include "pt_spectral.h"
#include "pt_scene_file.h"
int main(void) {
    pt_status (*m)(const pt_render_desc*, const pt_spectral_desc*, const pt_curve*, uint32_t, const float*, uint32_t, uint32_t, const int32_t*, int32_t, uint32_t, float*) = pt_spectral_response_matrix;
    pt_status (*p)(uint32_t, uint32_t, uint32_t, uint32_t, const float*, const float*, float*) = pt_spectral_project;
    pt_status (*r)(pt_scene*, uint32_t, const float*, float*) = pt_spectral_project_resident;
    pt_status (*q)(pt_scene*, uint32_t*, uint32_t*, uint32_t*) = pt_spectral_resident;
    pt_status (*c)(pt_scene_file*, const char*, pt_curve*, const float**, uint32_t*) = pt_scene_file_library_curve;
    printf("%d %d %d %d %d %d %d %zu %d\n", PT_SPECTRAL_MAX_RESPONSES, PT_SPECTRAL_MAX_SUBSAMPLES, PT_RESPONSE_CIE_X, PT_RESPONSE_CIE_Y, PT_RESPONSE_CIE_Z,
           PT_SPECTRAL_NO_FILTER, PT_SPECTRAL_MAX_BINS, sizeof(pt_curve), m && p && r && q && c);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t.o"), os.path.join(d, "t.c")])
        text = open(os.path.join(d, "t.c")).read().replace("int main(void) {", "int main(void) {\n#define pt_spectral_response_matrix 0\n#define pt_spectral_project 0\n"
                                                             "#define pt_spectral_project_resident 0\n#define pt_spectral_resident 0\n#define pt_scene_file_library_curve 0\n")
        open(os.path.join(d, "u.c"), "w").write(text.replace("m && p && r && q && c", "1"))       # (the same program without the libraries: it only prints)
        subprocess.check_call(["gcc", "-w", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "u"), os.path.join(d, "u.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "u")]).split()]
    assert out == [a.SPECTRAL_MAX_RESPONSES, a.SPECTRAL_MAX_SUBSAMPLES, a.RESPONSE_CIE_X, a.RESPONSE_CIE_Y, a.RESPONSE_CIE_Z, a.SPECTRAL_NO_FILTER, 64, C.sizeof(a.Curve), 1]
    assert out[:6] == [16, 16, -1, -2, -3, -1]
    L = pkg.load()
    assert L._spectral_response_matrix.argtypes[2:5] == [C.POINTER(a.Curve), C.c_uint32, f32p] and len(L._spectral_response_matrix.argtypes) == 11
    assert len(L._spectral_project.argtypes) == 7 and len(L._spectral_project_resident.argtypes) == 4 and len(L._spectral_resident.argtypes) == 4


@pytest.mark.parametrize("K", [1, 3, 8, 9, 16])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_emulated_projection_equals_the_numpy_restatement(emu_pj, B, K):
    """ptemu_spectral_project — the rule's text, grouped as the launcher groups the responses — over 37 pixels of random planes with both signs."""
    rng = np.random.default_rng(1000 * B + K)
    S, M = planes(rng, B, (1, 37)), weights(rng, K, B)
    out = np.full((K, 1, 37), 777.0, F)
    assert emu_pj.ptemu_spectral_project(37, 1, B, K, M.ctypes.data, S.ctypes.data, out.ctypes.data) == PT_OK, emu_pj.ptemu_spectral_project_last_error()
    assert np.array_equal(bits(out), bits(np_project(M, S)))
    # every k is a fold of its own: row k alone gives plane k
    k = K - 1
    one = np.zeros((1, 1, 37), F)
    assert emu_pj.ptemu_spectral_project(37, 1, B, 1, M[k:k + 1].copy().ctypes.data, S.ctypes.data, one.ctypes.data) == PT_OK
    assert np.array_equal(bits(one[0]), bits(out[k]))


def curve_scene(pkg):
    """The Cornell box's description with one tabulated (40 knots: it gets a cell table), one linear, one constant and one analytic curve added."""
    a = pkg.api
    b = pkg.scene.cornell_box()
    xs = np.linspace(370.0, 790.0, 40)
    b.curve_tabulated("sens_tab", xs, 0.2 + 0.7 * np.exp(-((xs - 540.0) / 60.0) ** 2))
    b.curve_linear("sens_lin", 380.0, 31.0, [0.1, 0.3, 0.8, 1.0, 0.9, 0.6, 0.5, 0.45, 0.3, 0.2, 0.15, 0.1])
    b._add_curve("sens_const", a.CURVE_CONST, 0, 0.625, 0.0)
    b.curve_cauchy("sens_cauchy", 1.5, 10000.0)
    return b


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("n", [1, 4, 16])
def test_response_matrix_equals_the_numpy_fold(emu, emu_pj, pkg, n, with_filter):  # noqa: F811
    """pt_spectral_response_matrix (host only: the library needs no device) and the emulation's copy of it against the fold of per-wavelength values from the
    emulation's curve evaluator and ptemu_xyz_bar: four curve kinds and the three CIE rows, 7 bins."""
    a = pkg.api
    lib = pkg.load()
    b = curve_scene(pkg)
    B = 7
    rd = a.render_desc(8, 8, 10, 3, wavelength=BOUNDS)
    names = ["sens_tab", "sens_lin", "sens_const", "sens_cauchy"]
    responses = names + [a.RESPONSE_CIE_X, a.RESPONSE_CIE_Y, a.RESPONSE_CIE_Z]
    filt = "cornell_white" if with_filter else None
    got = b.spectral_response_matrix(lib, rd, B, responses, filter=filt, subsamples=n)
    assert got.shape == (7, B) and got.dtype == F
    lam = np.zeros((B, n), F)
    assert emu_pj.ptemu_spectral_sample_lambdas(BOUNDS[0], BOUNDS[1], B, n, fptr(lam)) == PT_OK
    assert np.array_equal(bits(lam), bits(np_sample_lambdas(BOUNDS[0], BOUNDS[1], B, n)))
    centres = lib.spectral_bin_centres(rd, B)
    if n == 1:
        assert np.array_equal(bits(lam[:, 0]), bits(centres))
    sc = emu.create_scene(b)
    f = sc.curve_eval(b.curve(filt), lam.ravel()).reshape(B, n) if with_filter else None
    want = [np_matrix_row(sc.curve_eval(b.curve(name), lam.ravel()).reshape(B, n), f, n) for name in names]
    xb = xyz_bar(emu, lam)
    want += [np_matrix_row(np.ascontiguousarray(xb[..., c]), f, n) for c in range(3)]
    want = np.stack(want)
    assert np.all(np.isfinite(want)) and np.all(want[:4] > 0)
    assert np.array_equal(bits(got), bits(want))
    if n == 1 and not with_filter:
        assert np.array_equal(bits(got[4:]), bits(xyz_bar(emu, centres).T))
        assert np.array_equal(bits(lib.spectral_observer_matrix(rd, B)), bits(got[4:]))
    # the emulation's entry: the same numbers
    idx = [b.curve(r) if isinstance(r, str) else r for r in responses]
    carr = (a.Curve * len(b.curves))(*b.curves)
    cd = np.asarray(b.curve_data, F)
    rarr = (C.c_int32 * len(idx))(*idx)
    em = np.zeros((7, B), F)
    sd = a.SpectralDesc(B)
    st = emu_pj.ptemu_spectral_response_matrix(C.byref(rd), C.byref(sd), carr, len(b.curves), cd.ctypes.data, cd.size, 7, rarr, b.curve(filt) if with_filter else -1, n, em.ctypes.data)
    assert st == PT_OK, emu_pj.ptemu_spectral_project_last_error()
    assert np.array_equal(bits(em), bits(got))


def test_validation_rejects_each_rule_with_its_own_message(emu_pj, pkg):
    a = pkg.api
    msgs = {}
    S, M, out = np.ones((7, 2, 3), F), np.ones((3, 7), F), np.zeros((3, 2, 3), F)

    def project(key, w=3, h=2, bins=7, K=3, matrix=M, spectral=S, o=out):
        st = emu_pj.ptemu_spectral_project(w, h, bins, K, matrix.ctypes.data if matrix is not None else None, spectral.ctypes.data if spectral is not None else None,
                                           o.ctypes.data if o is not None else None)
        if st != PT_OK:
            assert st == PT_ERR_INVALID_ARGUMENT
            msgs.setdefault(key, set()).add(emu_pj.ptemu_spectral_project_last_error().decode())
        return st

    assert project("ok") == PT_OK and "ok" not in msgs
    bad = M.copy()
    for v in (np.nan, np.inf, -np.inf):
        bad[2, 6] = v
        assert project("p_finite", matrix=bad) != PT_OK
    big = np.ones((17, 65), F)
    assert project("p_spectral", spectral=None) != PT_OK and project("p_out", o=None) != PT_OK and project("p_matrix", matrix=None) != PT_OK
    assert project("p_k0", K=0) != PT_OK and project("p_k17", K=17, matrix=big) != PT_OK
    assert project("p_b0", bins=0) != PT_OK and project("p_b65", bins=65, matrix=big) != PT_OK
    assert project("p_size", w=0) != PT_OK and project("p_size", h=0) != PT_OK
    assert project("ok16", K=16, bins=64, matrix=big, spectral=np.ones((64, 2, 3), F), o=np.zeros((16, 2, 3), F)) == PT_OK
    # the resident entry's matrix check
    assert emu_pj.ptemu_spectral_check_matrix(3, 7, M.ctypes.data) == PT_OK
    assert emu_pj.ptemu_spectral_check_matrix(17, 7, big.ctypes.data) != PT_OK
    assert emu_pj.ptemu_spectral_project_last_error().decode() in msgs["p_k17"]

    rd = a.render_desc(8, 8, 10, 3)
    b = pkg.scene.cornell_box()
    carr = (a.Curve * len(b.curves))(*b.curves)
    cd = np.asarray(b.curve_data, F)
    mat = np.zeros((16, 64), F)

    def matrix(key, rdp=rd, bins=7, curves=carr, count=len(b.curves), data=cd, floats=cd.size, responses=(0, -1, -3), K=None, filt=-1, n=1, m=mat):
        sd = a.SpectralDesc(bins) if bins != "null" else None
        rarr = (C.c_int32 * max(len(responses), 1))(*responses) if responses is not None else None
        st = emu_pj.ptemu_spectral_response_matrix(C.byref(rdp) if rdp is not None else None, C.byref(sd) if sd is not None else None, curves, count,
                                                   data.ctypes.data if data is not None else None, floats, len(responses) if K is None else K, rarr, filt, n,
                                                   m.ctypes.data if m is not None else None)
        if st != PT_OK:
            assert st == PT_ERR_INVALID_ARGUMENT
            msgs.setdefault(key, set()).add(emu_pj.ptemu_spectral_project_last_error().decode())
        return st

    assert matrix("ok") == PT_OK and matrix("ok", responses=(-1, -2, -3), curves=None, count=0, data=None, floats=0) == PT_OK
    assert matrix("ok", filt=3, n=16) == PT_OK
    assert matrix("m_rd", rdp=None) != PT_OK and matrix("m_sd", bins="null") != PT_OK and matrix("m_responses", responses=None, K=3) != PT_OK
    assert matrix("m_matrix", m=None) != PT_OK and matrix("m_curves", curves=None) != PT_OK and matrix("m_data", data=None) != PT_OK
    assert matrix("m_b0", bins=0) != PT_OK and matrix("m_b65", bins=65) != PT_OK
    assert matrix("m_k0", responses=(), K=0) != PT_OK and matrix("m_k17", responses=(0,) * 17) != PT_OK
    assert matrix("m_n0", n=0) != PT_OK and matrix("m_n17", n=17) != PT_OK
    for r in (-4, len(b.curves), 2 ** 31 - 1, -2 ** 31):
        assert matrix("m_response", responses=(0, r)) != PT_OK
    for f in (-2, len(b.curves)):
        assert matrix("m_filter", filt=f) != PT_OK
    assert all(len(v) == 1 for v in msgs.values()), msgs
    flat = {k: next(iter(v)) for k, v in msgs.items()}
    # one message per rule, shared only where the rule is the same one (K and bins in both entries; a null matrix)
    same = [("p_k0", "m_k0"), ("p_k17", "m_k17"), ("p_b0", "m_b0"), ("p_b65", "m_b65"), ("p_matrix", "m_matrix")]
    for x, y in same:
        assert flat[x] == flat[y]
    distinct = [k for k in flat if k not in [y for _, y in same]]
    assert len({flat[k] for k in distinct}) == len(distinct), flat
    assert "16" in flat["p_k17"] and "64" in flat["p_b65"] and "finite" in flat["p_finite"] and "subsamples" in flat["m_n0"] and "16" in flat["m_n17"]
    assert "response 1" in flat["m_response"] and "filter" in flat["m_filter"] and "width" in flat["p_size"]
    # the product's entries run the same checks before they look for a device: refused as invalid arguments here, where there may be none
    lib = pkg.load()
    with pytest.raises(a.PtError, match="at most 16 responses"):
        lib.spectral_project(np.ones((7, 2, 3), F), np.ones((17, 7), F))
    with pytest.raises(a.PtError, match="not finite"):
        lib.spectral_project(np.ones((7, 2, 3), F), bad)
    with pytest.raises(a.PtError, match="subsamples"):
        lib.spectral_observer_matrix(rd, 7, subsamples=17)


def test_ptcli_refuses_bad_develop_arguments_while_parsing(pkg, tmp_path):
    """Each refusal exits with status 2 and its own message before any file is read; an unknown curve name fails once the scene file is loaded, naming it."""
    exe = ptcli(pkg)
    cases = [
        (["--develop", "cie"], "--develop needs --spectral-bins or --denoise-spectral-bins"),
        (["--spectral-bins", "8", "--develop-filter", "cornell_white"], "--develop-filter needs --develop"),
        (["--spectral-bins", "8", "--develop-subsamples", "4"], "--develop-subsamples needs --develop"),
        (["--spectral-bins", "8", "--develop", "a,b"], "--develop needs `cie` or three curve names"),
        (["--spectral-bins", "8", "--develop", "a,b,c,d"], "--develop needs `cie` or three curve names"),
        (["--spectral-bins", "8", "--develop", "a,,c"], "--develop needs `cie` or three curve names"),
        (["--spectral-bins", "8", "--develop", "cie", "--develop-subsamples", "0"], "--develop-subsamples needs a count in 1..16"),
        (["--spectral-bins", "8", "--develop", "cie", "--develop-subsamples", "17"], "--develop-subsamples needs a count in 1..16"),
        (["--spectral-bins", "8", "--develop", "cie", "--develop-subsamples", "x"], "--develop-subsamples needs a count in 1..16"),
    ]
    seen = set()
    for args, message in cases:
        r = subprocess.run([exe, "--config", "/nonexistent/config.toml"] + args, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 2 and ("error: " + message) in r.stderr, (args, r.stderr)
        seen.add(message)
    assert len(seen) == 5
    assert "--develop" in subprocess.run([exe, "--help"], capture_output=True, text=True).stderr
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    r = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n", "--spectral-bins", "8",
                        "--develop", "cornell_red,no_such_curve,cornell_white"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and "--develop" in r.stderr and "no_such_curve" in r.stderr, r.stderr
    ok = subprocess.run([exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg), "--output-dir", str(tmp_path / "out"), "-n", "--spectral-bins", "8",
                         "--develop", "srgb_r,srgb_g,srgb_b", "--develop-filter", "cornell_white"], capture_output=True, text=True, cwd=str(tmp_path))
    assert ok.returncode == 0, ok.stderr


def desc_bytes(d, pkg):
    """Everything a pt_scene_desc says: the struct's own bytes (counts, pointers excluded by comparing the arrays instead) and every array it points to."""
    a = pkg.api
    parts = [("env", bytes(d.environment)), ("esp", F(d.env_sampling_probability).tobytes())]
    for count, field in (("curve_count", "curves"), ("layer_count", "layers"), ("texstack_count", "texstacks"), ("material_count", "materials"), ("mesh_count", "meshes"),
                         ("instance_count", "instances"), ("camera_count", "cameras"), ("medium_count", "mediums")):
        n = getattr(d, count)
        p = getattr(d, field)
        parts.append((field, C.string_at(p, n * C.sizeof(p._type_)) if n else b""))
    for count, field, per in (("curve_data_count", "curve_data", 1), ("texture_data_count", "texture_data", 1), ("vertex_count", "vertices", 3), ("index_count", "indices", 1),
                              ("normal_count", "normals", 3), ("face_material_count", "face_materials", 1)):
        n = getattr(d, count) * per
        p = getattr(d, field)
        parts.append((field, C.string_at(p, n * C.sizeof(p._type_)) if n else b""))
    return parts


def test_library_curve_resolves_unused_curves_and_leaves_the_desc_alone(pkg, tmp_path):
    """The reference tree's cornell_box.toml: its curves library holds D65, which the scene does not use.  (The reference tree ships neither the box's OBJ nor
    cornell_light.csv — tests/test_reference_fixtures.py pins that — so this repository's copies are put where file names are looked up first: the working directory.)"""
    sf = pkg.scene_file
    data = os.path.join(pkg.PACKAGE_DIR, "data")
    for rel in ("meshes/cornell_box.obj", "meshes/cornell_box.mtl", "curves/csv/cornell_light.csv"):
        os.makedirs(os.path.dirname(str(tmp_path / "data" / rel)), exist_ok=True)
        shutil.copy(os.path.join(data, rel), str(tmp_path / "data" / rel))
    config = sf.Config(os.path.join(data, "config_cornell_c1.toml"))
    path = os.path.join(REF, "data", "scenes", "cornell_box.toml")
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    sf.set_root(REF)
    try:
        plain = sf.SceneFile(path, config)
        used = sf.SceneFile(path, config)
        assert used.curve("D65") == -1 and used.curve("cornell_white") >= 0        # lazily resolved: D65 is not in the scene
        before = desc_bytes(used.desc, pkg)
        c, d = used.library_curve("D65")
        assert c.kind == pkg.api.CURVE_TABULATED and c.data_offset == 0 and c.data_count > 100 and d.size == 2 * c.data_count
        csv = np.array([[float(v) for v in line.split(",")[:2]] for line in open(os.path.join(REF, "data", "curves", "csv", "D65.csv")).read().splitlines()
                        if re.match(r"\s*[-0-9.]", line)], F)
        assert np.array_equal(d[0::2], csv[:, 0])
        c2, d2 = used.library_curve("D65")                                           # a second request: the same curve
        assert bytes(c2) == bytes(c) and np.array_equal(d2, d)
        cw, dw = used.library_curve("cornell_white")                                 # one the scene does use: the same knots as the scene's
        sw = used.desc.curves[used.curve("cornell_white")]
        assert (cw.kind, cw.mode, cw.data_count) == (sw.kind, sw.mode, sw.data_count)
        assert np.array_equal(dw, np.ctypeslib.as_array(used.desc.curve_data, shape=(used.desc.curve_data_count,))[sw.data_offset:sw.data_offset + 2 * sw.data_count])
        with pytest.raises(sf.SceneFileError, match="no_such_curve"):
            used.library_curve("no_such_curve")
        after = desc_bytes(used.desc, pkg)
        assert after == before and used.curve("D65") == -1
        assert [(k, v) for k, v in desc_bytes(plain.desc, pkg)] == after
        assert used.desc.curve_count == plain.desc.curve_count
        # and the matrix helper over library names
        rd = pkg.api.render_desc(8, 8, 10, 3)
        m = used.spectral_response_matrix(pkg.load(), rd, 5, ["D65", "cornell_white"], filter="cornell_red", subsamples=2)
        assert m.shape == (2, 5) and np.all(np.isfinite(m)) and np.all(m > 0)
        assert desc_bytes(used.desc, pkg) == before
    finally:
        sf.set_root()
        os.chdir(cwd)


# ------------------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 1), (33, 9)])
def test_gpu_projection_bits(engine, w, h):
    """pt_spectral_project against the numpy restatement: one pixel, one lane more than a workgroup, a ragged 33x9; every B and K that takes another kernel form
    (K 1, 3, 8: one launch; 9, 16: two)."""
    for B in (1, 7, 64):
        for K in (1, 3, 8, 9, 16):
            rng = np.random.default_rng(100000 * w + 1000 * B + K)
            S, M = planes(rng, B, (h, w)), weights(rng, K, B)
            got = engine.spectral_project(S, M)
            assert got.shape == (K, h, w)
            assert np.array_equal(bits(got), bits(np_project(M, S))), (B, K)
    # a one-hot K = B matrix returns the planes (positive inputs: 0.0f + 1.0f * s, and the zero terms add +0)
    for B in (1, 7, 16):
        S = np.abs(planes(np.random.default_rng(B), B, (h, w)))
        assert np.array_equal(bits(engine.spectral_project(S, np.eye(B, dtype=F))), bits(S)), B


@pytest.mark.gpu
def test_gpu_resident_film_follows_the_last_spectral_render(engine, pkg):
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_box())
    rng = np.random.default_rng(5)
    assert sc.spectral_resident() is None
    with pytest.raises(a.PtError, match="no resident spectral film"):
        sc.spectral_project_resident(np.ones((3, 7), F))
    rd = a.render_desc(32, 32, 4, 4, seed=3, wavelength=BOUNDS)
    sc.render(rd)                                                              # (a plain render leaves no spectral film)
    assert sc.spectral_resident() is None
    first = {}
    for hero in (1, 4):
        rdh = a.render_desc(32, 32, 4, 4, seed=3, wavelength=BOUNDS, hero_wavelengths=hero)
        film, S, _ = sc.render_spectral(rdh, 7)
        first[hero] = (film.copy(), S.copy())
        assert sc.spectral_resident() == (32, 32, 7)
        for K in (3, 9):
            M = weights(rng, K, 7)
            got = sc.spectral_project_resident(M)
            assert got.shape == (K, 32, 32) and np.any(got != 0)
            assert np.array_equal(bits(got), bits(engine.spectral_project(S, M))), (hero, K)
        assert np.array_equal(bits(S), bits(first[hero][1]))
    # adaptive
    rda = a.render_desc(32, 32, 10, 4, seed=3, wavelength=BOUNDS)
    film_a, counts, S_a, _ = sc.render_adaptive_spectral(rda, 6, 30, 0.05)
    assert sc.spectral_resident() == (32, 32, 6)
    M = weights(rng, 9, 6)
    assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(engine.spectral_project(S_a, M)))
    with pytest.raises(ValueError):
        sc.spectral_project_resident(np.ones((3, 7), F))                       # (the earlier film's bins)
    with pytest.raises(a.PtError, match="at most 16 responses"):
        sc.spectral_project_resident(np.ones((17, 6), F))
    assert sc.spectral_resident() == (32, 32, 6)
    # a second, smaller render: the resident film is that one
    rd2 = a.render_desc(16, 8, 4, 4, seed=4, wavelength=BOUNDS)
    film2, S2, _ = sc.render_spectral(rd2, 5)
    assert sc.spectral_resident() == (16, 8, 5)
    M = weights(rng, 3, 5)
    got = sc.spectral_project_resident(M)
    assert got.shape == (3, 8, 16) and np.array_equal(bits(got), bits(engine.spectral_project(S2, M)))
    sc.render(rd)                                                              # a plain render and guides in between do not write the buffer
    sc.render_guides_bin_albedo(rd2, 5)
    assert sc.spectral_resident() == (16, 8, 5)
    assert np.array_equal(bits(sc.spectral_project_resident(M)), bits(got))
    # the renders themselves are what they were before any development ran
    for hero in (1, 4):
        rdh = a.render_desc(32, 32, 4, 4, seed=3, wavelength=BOUNDS, hero_wavelengths=hero)
        film, S, _ = sc.render_spectral(rdh, 7)
        assert film.tobytes() == first[hero][0].tobytes() and S.tobytes() == first[hero][1].tobytes()
    fresh = engine.create_scene(pkg.scene.cornell_box()).render_spectral(a.render_desc(32, 32, 4, 4, seed=3, wavelength=BOUNDS), 7)
    assert fresh[0].tobytes() == first[1][0].tobytes() and fresh[1].tobytes() == first[1][1].tobytes()
    assert sc.render(rd)[0].tobytes() == first[1][0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4])
def test_gpu_matrix_is_the_fold_of_the_devices_curve_values(engine, pkg, n):
    """The host matrix over the Cornell scene's own curves against the fold of Scene.curve_eval, the device's evaluator: the host runs the same lane code."""
    a = pkg.api
    b = pkg.scene.cornell_box()
    sc = engine.create_scene(b)
    B = 7
    rd = a.render_desc(8, 8, 10, 3, wavelength=BOUNDS)
    names = ["cornell_white", "cornell_green", "cornell_red", "cornell_light", "flat_78"]
    lam = np_sample_lambdas(BOUNDS[0], BOUNDS[1], B, n)
    for filt in (None, "cornell_white"):
        got = b.spectral_response_matrix(engine, rd, B, names, filter=filt, subsamples=n)
        f = sc.curve_eval(b.curve(filt), lam.ravel()).reshape(B, n) if filt else None
        want = np.stack([np_matrix_row(sc.curve_eval(b.curve(name), lam.ravel()).reshape(B, n), f, n) for name in names])
        assert np.all(want > 0)
        assert np.array_equal(bits(got), bits(want)), filt


def cie_fit_constants():
    """The Gaussians of the colour-matching fit, from csrc/pt_device.h (xyz_bar_contract): per channel a list of (alpha, mu, s1, s2), in angstrom."""
    text = open(os.path.join(CSRC, "pt_device.h")).read()
    body = re.search(r"PT_HD void xyz_bar_contract\(.*?\n\}", text, re.S).group(0)
    fit = []
    for ch in ("xb", "yb", "zb"):
        line = re.search(r"\*%s = (.*);" % ch, body).group(1)
        fit.append([tuple(float(v) for v in g) for g in re.findall(r"gaussian64\(a, ([-0-9.]+), ([-0-9.]+), ([-0-9.]+), ([-0-9.]+)\)", line)])
    assert [len(c) for c in fit] == [3, 2, 2]
    return fit


def developed_bound(B, spp, T):
    """Per channel: L_c * (w / 2) * T + R_c * T.  L_c: a Gaussian alpha * exp(-((x - mu) / s)^2 / 2) has slope at most |alpha| / (s * sqrt(e)), so the fit's
    Lipschitz constant is at most the sum of |alpha_i| / (min(s1_i, s2_i) * sqrt(e)) per angstrom, times 10 per nm; a sample in bin b is at most w / 2 from the
    centre.  R_c = (spp + B + 8) * 2^-23 * sum |alpha_i|: the rounding of the two f32 folds (spp additions in the film, B in the development, and a few
    operations around them), each relative to a sum bounded by sum |alpha_i| * T."""
    w = (BOUNDS[1] - BOUNDS[0]) / B
    out = []
    for ch in cie_fit_constants():
        L = 10.0 * sum(abs(al) / (min(s1, s2) * np.sqrt(np.e)) for al, mu, s1, s2 in ch)
        R = (spp + B + 8) * 2.0 ** -23 * sum(abs(al) for al, mu, s1, s2 in ch)
        out.append(L * (w / 2.0) * T + R * T)
    return np.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("hero", [1, 4])
def test_gpu_the_developed_picture_is_the_film(engine, pkg, hero):
    """Cornell box 24x24, 20 spp: the bins developed with the colour-matching rows at the bin centres are the XYZ film up to the variation of the fit inside a
    bin and the rounding of the two folds — a derived bound, per pixel and channel, that shrinks with the bin width."""
    a = pkg.api
    sc = engine.create_scene(pkg.scene.cornell_box())
    spp = 20
    rd = a.render_desc(24, 24, spp, 4, seed=11, wavelength=BOUNDS, hero_wavelengths=hero)
    worst = {}
    for B in (16, 64):
        film, S, _ = sc.render_spectral(rd, B)
        assert np.all(S >= 0) and np.any(S > 0)
        P = sc.spectral_project_resident(engine.spectral_observer_matrix(rd, B, subsamples=1))
        T = S.astype(np.float64).sum(0)
        bound = developed_bound(B, spp, T)
        err = np.abs(P.astype(np.float64) - np.moveaxis(film[..., :3], -1, 0).astype(np.float64))
        print("B = %d hero = %d: largest |P - F| / bound per channel %s" % (B, hero, [float((err[c][T > 0] / bound[c][T > 0]).max()) for c in range(3)]))
        assert np.all(err <= bound), (B, [float((err[c] - bound[c]).max()) for c in range(3)])
        assert np.all(P[:, T == 0] == 0)
        worst[B] = developed_bound(B, spp, 1.0)
    assert np.all(worst[64] < worst[16])


@pytest.mark.gpu
def test_gpu_ptcli_develop(engine, pkg, tmp_path):
    """ptcli --spectral-bins 8 --develop cie writes <name>_developed.exr / .png beside files that stay byte for byte; the EXR is the Python path's; three named
    curves behind a filter give another picture."""
    sf = pkg.scene_file
    exe = ptcli(pkg)
    cfg = tmp_path / "config.toml"
    cfg.write_text(scaled_c2_config(pkg))
    base = [exe, "--root", pkg.PACKAGE_DIR, "--config", str(cfg)]

    def run(out, *extra):
        return subprocess.run(base + ["--output-dir", str(tmp_path / out)] + list(extra), capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    spec, dev = run("spec", "--spectral-bins", "8"), run("dev", "--spectral-bins", "8", "--develop", "cie")
    cam = run("cam", "--spectral-bins", "8", "--develop", "srgb_r,srgb_g,srgb_b", "--develop-filter", "cornell_white", "--develop-subsamples", "4")
    for r in (spec, dev, cam):
        assert r.returncode == 0, r.stdout + r.stderr
    assert "beauty_developed.exr" in dev.stdout
    assert sorted(os.listdir(str(tmp_path / "spec"))) == ["beauty.exr", "beauty.png", "beauty_spectral.exr"]
    assert sorted(os.listdir(str(tmp_path / "dev"))) == ["beauty.exr", "beauty.png", "beauty_developed.exr", "beauty_developed.png", "beauty_spectral.exr"]
    for name in ("beauty.exr", "beauty.png", "beauty_spectral.exr"):
        assert (tmp_path / "spec" / name).read_bytes() == (tmp_path / "dev" / name).read_bytes() == (tmp_path / "cam" / name).read_bytes(), name
    config = sf.Config(str(cfg))
    rd, od = config.render_desc(0, seed=1), config.output_desc(0)
    sc = engine.create_scene(sf.SceneFile(os.path.join(pkg.PACKAGE_DIR, config.scene_file), config))
    film, spectral, _ = sc.render_spectral(rd, 8)
    P = engine.spectral_project(spectral, engine.spectral_observer_matrix(rd, 8))
    packed = np.concatenate([np.moveaxis(P, 0, -1), np.zeros(P.shape[1:] + (1,), F)], axis=-1)
    rgba, linear = engine.output_film(packed, od.tonemap, od.luminance_only, od.exposure, od.key_value, od.white_point, od.colorspace, od.factor)
    engine.write_exr(str(tmp_path / "python.exr"), linear, od.colorspace)
    engine.write_png(str(tmp_path / "python.png"), rgba, od.colorspace)
    assert (tmp_path / "python.exr").read_bytes() == (tmp_path / "dev" / "beauty_developed.exr").read_bytes()
    assert (tmp_path / "python.png").read_bytes() == (tmp_path / "dev" / "beauty_developed.png").read_bytes()
    assert (tmp_path / "cam" / "beauty_developed.exr").read_bytes() != (tmp_path / "dev" / "beauty_developed.exr").read_bytes()
    assert len((tmp_path / "cam" / "beauty_developed.exr").read_bytes()) == len((tmp_path / "dev" / "beauty_developed.exr").read_bytes())
    # with the joint denoiser: the undenoised and the denoised bins, through the host-array entry; the other files stay what --develop-less runs write
    plain = run("dn", "--denoise", "--denoise-spectral-bins", "8")
    both = run("dn_dev", "--denoise", "--denoise-spectral-bins", "8", "--develop", "cie")
    assert plain.returncode == 0 and both.returncode == 0, plain.stderr + both.stderr
    before = sorted(os.listdir(str(tmp_path / "dn")))
    assert sorted(os.listdir(str(tmp_path / "dn_dev"))) == sorted(before + ["beauty_developed.exr", "beauty_developed.png", "beauty_denoised_developed.exr", "beauty_denoised_developed.png"])
    for name in before:
        assert (tmp_path / "dn" / name).read_bytes() == (tmp_path / "dn_dev" / name).read_bytes(), name
    assert (tmp_path / "dn_dev" / "beauty_developed.exr").read_bytes() == (tmp_path / "dev" / "beauty_developed.exr").read_bytes()     # (the same bins: a fixed count)
    assert (tmp_path / "dn_dev" / "beauty_denoised_developed.exr").read_bytes() != (tmp_path / "dn_dev" / "beauty_developed.exr").read_bytes()
