"""Film output and film comparison against tests/film_reference.py, an f64 reading of the reference's Rust that shares nothing
with the oracle or the engine.

CPU tier: the oracle against the reading for every tonemapper x luminance-only x colour space, two parameter sets, at 96x96
and 1024x1024; the error model's power to reject six wrong readings; the non-finite cases one by one; the comparison tool; and
the PNG / EXR writers (host code: binding the engine library does not touch a device).  GPU tier: the engine against the
reading at sizes where the grid-stride loops run zero, one and several iterations per lane, the same non-finite cases, and the
comparison tool bit for bit.  Every tonemapped film of at least 64x64 must keep 64 distinct codes and 90 % non-black pixels, so
that a poisoned film cannot make a case vacuous."""
import itertools
import struct

import numpy as np
import pytest

import film_reference as fr

COMBOS = list(itertools.product((fr.CLAMP, fr.REINHARD0, fr.REINHARD1), (True, False), (fr.SRGB, fr.REC709, fr.REC2020)))
PARAMS = {"defaults": {}, "alt": dict(exposure=1.5, factor=0.25, white_point=0.5, key_value=0.3)}
GPU_SIZES = [(1, 1), (1, 7), (300, 1), (61, 97), (512, 512), (512, 513), (317, 1021), (1024, 1024), (1024, 2048)]   # (h, w)
P = (3, 5)


@pytest.fixture(scope="module")
def base(pkg, oracle):
    """A 256x256 Cornell box from the oracle: the tile every larger film is made of."""
    film, _ = oracle.create_scene(pkg.scene.cornell_box()).render(pkg.api.render_desc(256, 256, 4, 4))
    return film


@pytest.fixture(scope="module")
def film96(pkg, oracle):
    film, _ = oracle.create_scene(pkg.scene.cornell_box()).render(pkg.api.render_desc(96, 96, 8, 4))
    return film


def tiled(base, h, w):
    """An h x w film of 256x256 tiles, tile k scaled by 2^(k mod 16 / 4 - 2): a dynamic range no single render has."""
    th, tw = -(-h // 256), -(-w // 256)
    rows = [np.concatenate([base * np.float32(2.0 ** ((r * tw + c) % 16 / 4.0 - 2.0)) for c in range(tw)], 1) for r in range(th)]
    return np.ascontiguousarray(np.concatenate(rows, 0)[:h, :w], np.float32)


def run_oracle(oracle, pkg):
    from test_output import oracle_output
    return lambda film, **kw: oracle_output(oracle, pkg, film, **kw)


def check_case(run, film, kw):
    ref = fr.output_film(film, **kw)
    rgba, lin = run(film, **kw)
    v = fr.check_output(ref, rgba, lin)
    assert not any(v.values()), (kw, v)
    if film.shape[0] >= 64 and film.shape[1] >= 64:
        distinct, lit = fr.non_degenerate(rgba)
        assert distinct >= 64 and lit >= 0.9, (kw, distinct, lit)
    return ref, rgba


def case(tm, lo, cs, params):
    return dict(params, tonemap=tm, luminance_only=lo, colorspace=cs)


# ---- CPU tier ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", list(PARAMS))
@pytest.mark.parametrize("size", [96, 1024])
def test_oracle_output_matches_reference(pkg, oracle, base, film96, size, params):
    film = film96 if size == 96 else tiled(base, size, size)
    run = run_oracle(oracle, pkg)
    for tm, lo, cs in COMBOS:
        check_case(run, film, case(tm, lo, cs, PARAMS[params]))


def test_error_model_rejects_wrong_readings(base):
    """Each wrong reading of output_film, quantised as an implementation would, must fail check_output."""
    film = tiled(base, 1024, 1024)
    n = film.shape[0] * film.shape[1]

    def rejected(kw, **wrong):
        codes = fr.output_film(film, **dict(kw, **wrong)).codes
        rgba = np.concatenate([codes, np.full(film.shape[:2] + (1,), 255, np.uint8)], -1)
        return fr.check_output(fr.output_film(film, **kw), rgba)["codes"]
    for tm in (fr.REINHARD0, fr.REINHARD1):
        kw = case(tm, False, fr.REC2020, {})
        assert rejected(kw) == 0                                                              # the reading passes itself
        assert rejected(kw, lw=fr.log_average(film, tm, False, 1.0, fold=False)) > 100        # x3: the exact f64 sum
    for tm, lo in ((fr.REINHARD0, True), (fr.REINHARD1, True), (fr.REINHARD1, False)):
        kw = case(tm, lo, fr.SRGB, {})
        lw = fr.log_average(film, tm, lo, 1.0)
        assert rejected(kw, lw=lw * (1 + 1e-4)) > 100
        assert rejected(kw, lw=fr.log_average(film, tm, lo, 1.0, leave_out=np.arange(n // 2, n // 2 + 256))) > 100
    assert rejected(case(fr.CLAMP, True, fr.SRGB, {}), quantize="round") > 100
    assert rejected(case(fr.REINHARD0, True, fr.REC2020, {}), matrix=fr.M709) > 100
    assert rejected(case(fr.REINHARD0, True, fr.REC709, {}), oetf_params=fr.OETF_SRGB) > 100


def test_log_average_is_the_reference_fold(base):
    """The x3 l_w is the sequential f32 fold, which at 1024x1024 is far from the exact sum."""
    film = tiled(base, 1024, 1024)
    t = fr.log_terms_x3(film)
    s = np.float32(0.0)
    for v in t[:4096, 1]:                                           # np.cumsum(dtype=float32) is a left fold
        s = np.float32(s + v)
    assert s == np.cumsum(t[:4096, 1], dtype=np.float32)[-1]
    fold, exact = fr.log_average(film, fr.REINHARD1, False, 1.0), fr.log_average(film, fr.REINHARD1, False, 1.0, fold=False)
    assert (np.abs(fold / exact - 1) > 1e-3).any()


MAUVE_MAP = {(fr.CLAMP, True): fr.MAUVE / fr.MAUVE[1], (fr.CLAMP, False): np.minimum(fr.MAUVE, 1.0), (fr.REINHARD1, False): fr.MAUVE}
POISONS = [("nan_lum", 1, np.nan), ("inf_lum", 1, np.inf), ("nan_x", 0, np.nan), ("inf_x", 0, np.inf), ("ninf_x", 0, -np.inf),
           ("inf_z", 2, np.inf), ("ninf_z", 2, -np.inf)]


def check_nonfinite(film, run):
    """One non-finite value at pixel P, for the six tonemapper forms (sRGB, default parameters): what the reference does,
    stated against the reading, then the implementation against the reading."""
    w = film.shape[1]
    others = np.ones(film.shape[:2], bool); others[P] = False
    for name, ch, val in POISONS:
        f = film.copy(); f[P + (ch,)] = val
        for tm, lo in itertools.product((fr.CLAMP, fr.REINHARD0, fr.REINHARD1), (True, False)):
            kw = dict(tonemap=tm, luminance_only=lo)
            ref, clean = fr.output_film(f, **kw), fr.output_film(film, **kw)
            x3 = tm != fr.CLAMP and not lo
            mauve = MAUVE_MAP.get((tm, lo))
            at_p = "mauve" if (tm, lo) in MAUVE_MAP else "black"
            if name == "nan_lum":                                   # skipped by the sum, the divisor is still n
                if tm != fr.CLAMP:
                    assert np.array_equal(ref.lw, fr.log_average(film, tm, lo, 1.0, leave_out=[P[0] * w + P[1]]))
            elif name == "inf_lum" and tm != fr.CLAMP:              # l_w = inf
                assert np.isinf(ref.lw[1])
                if lo:
                    assert (ref.codes == 0).all()                   # every Reinhard pixel black
                else:
                    assert (ref.xyz[others][:, 1] == 0).all()
            elif x3 and (np.isnan(val) or val < 0):                  # ln(NaN), ln(-inf): l_w[ch] is NaN for the whole film
                assert np.isnan(ref.lw[ch])
                if tm == fr.REINHARD0:
                    assert (ref.codes == 0).all()
                else:
                    assert (ref.xyz == fr.MAUVE).all()
                at_p = None
            elif x3:                                                # +inf in X or Z: l_w[ch] = inf, that channel maps to 0
                assert np.isinf(ref.lw[ch]) and (ref.xyz[others][:, ch] == 0).all()
            else:                                                   # luminance only, or Clamp: only P changes
                assert np.array_equal(ref.lw, clean.lw) and np.array_equal(ref.codes[others], clean.codes[others])
                at_p = "mauve" if mauve is not None else "scaled mauve"
            if at_p == "black":
                assert np.isnan(ref.s[P]).all() and (ref.codes[P] == 0).all()
            elif at_p == "mauve":
                assert np.allclose(ref.xyz[P], mauve, rtol=1e-12)
            elif at_p == "scaled mauve":                            # sf (from the finite luminance) times MAUVE
                assert np.allclose(ref.xyz[P] / fr.MAUVE, ref.xyz[P][1] / fr.MAUVE[1], rtol=1e-12)
            rgba, lin = run(f, **kw)
            v = fr.check_output(ref, rgba, lin)
            assert not any(v.values()), (name, kw, v)


def test_oracle_nonfinite_semantics(pkg, oracle, film96):
    check_nonfinite(film96, run_oracle(oracle, pkg))


def compare_images(h, w, seed=5):
    rng = np.random.default_rng(seed)
    truth = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    image = (truth + rng.normal(0, 0.05, (h, w, 4))).astype(np.float32)
    if h * w >= 16:
        truth[0, -1, 1] = 0.0; truth[-1, 0] = 0.0; image[-1, 0, 2] = 0.0      # truth == 0: |d| / 0 -> 0, 0 / 0 -> 0
        image[h // 2, w // 2, 0] = np.nan; truth[-1, -1, 3] = np.inf; image[0, 0, 1] = -np.inf
    return image, truth


def compare_edge_cases():
    one = np.zeros((3, 4, 4), np.float32)
    nan = np.full((3, 4, 4), np.nan, np.float32)
    single = nan.copy(); single[1, 2] = [0.5, 0.25, 1.0, 0.0]
    zero_t = np.ones((3, 4, 4), np.float32); zero_t[..., 1] = 0.0; zero_t[0, 0] = 0.0
    img = np.full((3, 4, 4), 0.75, np.float32); img[0, 0, 2] = 0.0
    return {"all_nonfinite": (nan, one), "identical": (one + 0.25, one + 0.25), "single_finite": (single, one),
            "zero_truth": (img, zero_t)}


def check_compare(run, image, truth, mode, label="", rtol=1e-12):
    """rtol bounds mean_abs and rmse against the exact sums: 1e-12 for the engine's sums of per-lane partials; the oracle's
    sequential f64 sum of n non-negative terms is within n 2^-53 (relative), which is larger at 1024x1024."""
    ref = fr.compare_films(image, truth, mode)
    out, st = run(image, truth, mode)
    if mode == fr.RMSE:
        assert np.abs(out.astype(np.float64) - ref.colours).max() <= 1e-6, label
    else:
        bits, want = out.view(np.uint32), ref.out.view(np.uint32)
        assert np.array_equal(np.isnan(out), np.isnan(ref.out)), label
        assert np.array_equal(bits[~np.isnan(out)], want[~np.isnan(ref.out)]), label
    assert list(st.linf) == list(ref.linf) and st.nonfinite == ref.nonfinite, label
    assert st.pixel_min == ref.pixel_min and st.pixel_max == ref.pixel_max, label        # the per-pixel value, exactly
    assert np.allclose(list(st.mean_abs), ref.mean_abs, rtol=rtol, atol=0) and np.isclose(st.rmse, ref.rmse, rtol=rtol, atol=0), label
    return ref, out, st


def check_compare_edges(run):
    e = compare_edge_cases()
    violet = np.array([0x44, 0x01, 0x54]) / 255.0
    for mode in (fr.ABSOLUTE, fr.RMSE, fr.RELATIVE):
        for name, (image, truth) in e.items():
            ref, out, st = check_compare(run, image, truth, mode, (name, mode))
            if name == "all_nonfinite":
                assert st.nonfinite == 12 and st.rmse == 0 and max(st.linf) == 0 and max(st.mean_abs) == 0 and st.pixel_max == 0
            if name == "identical" and mode == fr.RMSE:           # hi == lo: every pixel at t = 0
                assert np.allclose(out[..., :3], violet, atol=1e-6, rtol=0) and (out[..., 3] == 1).all()
            if name == "single_finite":
                assert st.nonfinite == 11 and list(st.linf) == [0.5, 0.25, 1.0, 0.0]
                if mode == fr.RMSE:
                    assert np.allclose(out[1, 2, :3], violet, atol=1e-6, rtol=0)
            if name == "zero_truth" and mode == fr.RELATIVE:
                assert (out[..., 1] == 0).all() and (out[0, 0] == 0).all() and np.allclose(out[1:, :, 0], 0.25)


def test_oracle_compare_matches_reference(pkg, oracle):
    run = lambda a, b, m: oracle.compare_films(a, b, m)
    for h, w in ((1, 1), (1024, 1024)):
        image, truth = compare_images(h, w)
        for mode in (fr.ABSOLUTE, fr.RMSE, fr.RELATIVE):
            check_compare(run, image, truth, mode, (h, w, mode), rtol=max(1e-12, 4 * h * w * 2.0 ** -53))
    check_compare_edges(run)


def test_viridis_reading():
    """The B-spline's end points are the end keys; at t = 1/2 it lies within a few percent of the middle key #26838f."""
    v = fr.viridis(np.array([0.0, 0.5, 1.0]))
    assert np.allclose(v[0], [0x44 / 255, 0x01 / 255, 0x54 / 255], atol=1e-12) and np.allclose(v[2], [0xfe / 255, 0xe8 / 255, 0x25 / 255], atol=1e-12)
    assert np.allclose(v[1], np.array([0x26, 0x83, 0x8f]) / 255.0, atol=0.03)


def stored_blocks(z):
    """The zlib stream's stored deflate blocks: [(final, length)], checking each LEN / NLEN pair."""
    assert z[0] == 0x78 and (z[0] * 256 + z[1]) % 31 == 0
    pos, blocks = 2, []
    while True:
        final, btype = z[pos] & 1, (z[pos] >> 1) & 3
        n, nn = struct.unpack("<HH", z[pos + 1:pos + 5])
        assert btype == 0 and n ^ nn == 0xffff
        blocks.append((final, n)); pos += 5 + n
        if final:
            break
    assert pos + 4 == len(z)
    return blocks


@pytest.mark.parametrize("h,w", [(1, 1), (120, 150), (1, 16384), (1024, 1024)])
def test_png_writer(pkg, engine, tmp_path, h, w):
    from test_output import read_png
    rgba = np.random.default_rng(h * w).integers(0, 256, (h, w, 4), dtype=np.uint8)
    path = str(tmp_path / "out.png")
    engine.write_png(path, rgba, pkg.api.COLORSPACE_SRGB)
    back, chunks = read_png(path)                                  # CRCs checked; zlib checks the Adler-32
    assert np.array_equal(back, rgba)
    data = open(path, "rb").read()
    i = data.index(b"IDAT")
    z = data[i + 4:i + 4 + struct.unpack(">I", data[i - 4:i])[0]]
    blocks = stored_blocks(z)
    raw = h * (4 * w + 1)
    assert len(blocks) == -(-raw // 65535) and sum(n for _, n in blocks) == raw
    assert all(n == 65535 for _, n in blocks[:-1]) and [f for f, _ in blocks] == [0] * (len(blocks) - 1) + [1]
    assert struct.unpack(">I", chunks[b"gAMA"])[0] == round(100000 / 2.2)


def test_exr_writer(pkg, engine, tmp_path):
    h, w = 317, 1021
    lin = np.random.default_rng(7).normal(0, 1, (h, w, 3)).astype(np.float32)
    path = str(tmp_path / "out.exr")
    engine.write_exr(path, lin, pkg.api.COLORSPACE_REC709)
    d = open(path, "rb").read()
    end = d.index(b"screenWindowWidth\0float\0") + len(b"screenWindowWidth\0float\0") + 4 + 4 + 1
    offs = np.frombuffer(d[end:end + 8 * h], "<u8")
    assert np.array_equal(offs, end + 8 * h + (8 + 12 * w) * np.arange(h, dtype=np.uint64))
    assert len(d) == end + 8 * h + (8 + 12 * w) * h
    for y in range(h):
        yy, sz = struct.unpack("<ii", d[offs[y]:offs[y] + 8])
        assert yy == y and sz == 12 * w
        row = np.frombuffer(d[offs[y] + 8:offs[y] + 8 + sz], "<f4").reshape(3, w)
        assert np.array_equal(row, lin[y].T[::-1])                 # B, G, R


# ---- GPU tier ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("params", list(PARAMS))
def test_engine_output_1024(engine, base, params):
    film = tiled(base, 1024, 1024)
    for tm, lo, cs in COMBOS:
        check_case(engine.output_film, film, case(tm, lo, cs, PARAMS[params]))


@pytest.mark.gpu
@pytest.mark.parametrize("hw", GPU_SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_engine_output_sizes(engine, base, hw):
    """Six of the 36 cases per size, a different six at each size."""
    h, w = hw
    film = tiled(base, h, w)
    k = GPU_SIZES.index(hw)
    for j in range(6):
        tm, lo, cs = COMBOS[(5 * k + 3 * j) % len(COMBOS)]
        check_case(engine.output_film, film, case(tm, lo, cs, PARAMS[list(PARAMS)[(k + j) % 2]]))


@pytest.mark.gpu
def test_engine_nonfinite_semantics(engine, film96):
    check_nonfinite(film96, engine.output_film)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", GPU_SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_engine_compare_matches_reference(engine, hw):
    image, truth = compare_images(*hw)
    for mode in (fr.ABSOLUTE, fr.RMSE, fr.RELATIVE):
        check_compare(engine.compare_films, image, truth, mode, (hw, mode))


@pytest.mark.gpu
def test_engine_compare_edge_cases(engine):
    check_compare_edges(engine.compare_films)
