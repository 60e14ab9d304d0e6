"""An independent float64 reading of the film output stage and of the comparison tool, written from the reference's Rust alone
(line numbers below) and sharing no code, header or structure with oracle/ptref.cpp, csrc/pt_output.hip or csrc/pt_compare.hip:

  * output_film (src/renderer/mod.rs:24-80): Tonemapper::initialize (the log-average l_w), Tonemapper::map, XYZ -> linear RGB,
    the OETF and the 8-bit quantisation of write_to_files (src/tonemap/mod.rs:207-333), and the linear RGB of its EXR (:225-246);
  * compare_films: the three modes of src/bin/compare_exr.rs:70-162 and the statistics of pt_compare_films (include/pt_api.h);
  * check_output: the error model an f32 implementation of output_film is held to against this reading.

Per-pixel maths is f64.  What the reference decides in f32 is kept in f32 where the decision or the value depends on it: the
x3 log-average is its f32 left fold, and the compare stage's per-pixel outputs are single f32 operations."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of f32
CLAMP, REINHARD0, REINHARD1 = 0, 1, 2
SRGB, REC709, REC2020 = 0, 1, 2
ABSOLUTE, RMSE, RELATIVE = 0, 1, 2

MAUVE = np.array([0.5199467, 51.48687, 1.0180528], F32).astype(np.float64)     # src/lib.rs:45
M709 = np.array([[3.24096994, -1.53738318, -0.49861076], [-0.96924364, 1.8759675, 0.04155506],
                 [0.05563008, -0.20397696, 1.05697151]], F32).astype(np.float64)  # XYZ_TO_REC709_LINEAR, tonemap/mod.rs:23-33
M2020 = np.array([[1.4628067, -0.1840623, -0.2743606], [-0.5217933, 1.4472381, 0.0677227],
                  [0.0349342, -0.0968930, 1.2884099]], F32).astype(np.float64)    # XYZ_TO_REC2020_LINEAR, :36-39
# OETFs (tonemap/mod.rs:153-159 sRGB, :173-180 Rec709 and :193-200 Rec2020, the same curve): (knee, slope below it, a, gamma, b)
# for v < knee ? slope v : a v^gamma - b; the f32 literals of the Rust source, evaluated in f64
OETF_SRGB = tuple(float(F32(v)) for v in (0.0031308, 323.0 / 25.0, 211.0 / 200.0, 5.0 / 12.0, 11.0 / 200.0))
OETF_REC709 = tuple(float(F32(v)) for v in (0.01805397, 4.5, 1.0992968, 0.45, 0.09929682))

# The error model.  An f32 implementation rounds each operation to within U relative.  EPS_OPS bounds, relative to the scale
# of check_output's E, the longest chain: the Reinhard1 x3 map (8 roundings: key c, / l_w, mul l, + 1, l (..), 1 + l, the
# division, sf c), a 3x3 matrix row (3 roundings of at most sum_j |m_ij o_j|), and the OETF's power branch (powf accurate to
# 2 ulp, then a v^g, - b and * 255, 3 roundings; each is relative to a v^g = (v OETF'(v)) / g, g >= 0.41, so about 12 U in
# units of |v| OETF'(v)), together 23 U, rounded up to 32 U.  EPS_LW is the log-average's term: the reference rounds l_w to
# f32 (exp in f32 for x3, then / factor), at most 4 U, and Reinhard1's map amplifies a relative error of l_w at most twice
# (d ln sf / d ln l = 1 + m l / (1 + m l) - l / (1 + l) < 2): 8 U = 4.8e-7, bounded by 1e-6.
EPS_OPS = 32 * U
EPS_LW = 1e-6
EPS = EPS_OPS + EPS_LW


def log_terms_x3(film):
    """(f32x4::splat(DELTA) + color.0).ln() of every pixel, correctly rounded to f32 (reinhard0.rs:150, reinhard1.rs:158)."""
    c = np.asarray(film, F32).reshape(-1, 4)[:, :3]
    with np.errstate(all="ignore"):
        return np.log((F32(0.001) + c).astype(np.float64)).astype(F32)


def log_average(film, tonemap, luminance_only, factor, fold=True, leave_out=None):
    """l_w (f64, three channels) of Tonemapper::initialize: pixels whose luminance is NaN are skipped, the divisor is every
    pixel.  Luminance only: an f64 sum of ln(0.001 + (f64)lum) (reinhard0.rs:43) or of ln((f64)(0.001f + lum))
    (reinhard1.rs:45), then exp(sum / n) / factor (reinhard0.rs:66, reinhard1.rs:68).  x3: the f32 left fold in row-major
    order (reinhard0.rs:140-161, reinhard1.rs:149-169), then exp(sum / (f32)n) / factor (reinhard0.rs:173, reinhard1.rs:181).
    fold=False (an exact f64 sum of the x3 terms) and leave_out (pixel indices skipped by the sum) are the sensitivity tests'
    wrong readings."""
    f = np.asarray(film, F32).reshape(-1, 4)
    n = f.shape[0]
    skip = np.isnan(f[:, 1])
    if leave_out is not None:
        skip = skip.copy(); skip[leave_out] = True
    with np.errstate(all="ignore"):
        if luminance_only:
            y = f[~skip, 1]
            terms = np.log(0.001 + y.astype(np.float64)) if tonemap == REINHARD0 else np.log((F32(0.001) + y).astype(np.float64))
            return np.full(3, np.exp(terms.sum() / n) / factor)
        t = log_terms_x3(f)
        t[skip] = 0.0
        s = np.cumsum(t, axis=0, dtype=F32)[-1] if fold else t.astype(np.float64).sum(axis=0).astype(F32)
        return np.exp((s / F32(n)).astype(np.float64)) / factor


def map_pixels(film, tonemap, luminance_only, exposure, key_value, white_point, factor, lw):
    """Tonemapper::map in f64 (XYZ, [..., 3]).  The MAUVE rules test finiteness at different points: Clamp on the film times
    factor, before the map (clamp.rs:78-81); Reinhard0, Reinhard1 and Reinhard0x3 on the film pixel, after the scaling factor
    was computed from it (reinhard0.rs:92-100,200-208, reinhard1.rs:97-108); Reinhard1x3 on the mapped value (reinhard1.rs:
    220-231).  The film's fourth lane is 0 and takes no part."""
    f = np.asarray(film, F32)[..., :3]
    c = f.astype(np.float64)
    with np.errstate(all="ignore"):
        if tonemap == CLAMP:
            ok = np.isfinite(f * F32(factor)).all(-1)[..., None]     # the f32 product decides
            c = np.where(ok, c * float(F32(factor)), MAUVE)
            e = 2.0 ** float(F32(exposure))
            if luminance_only:
                lum = c[..., 1:2]
                return np.clip(lum * e, 0.0, 1.0) / lum * c
            return np.clip(c * e, 0.0, 1.0)
        ok = np.isfinite(f).all(-1)[..., None]
        key, mul = float(F32(key_value)), 1.0 / float(F32(white_point)) ** 2

        def scale(l):
            return l / (1.0 + l) if tonemap == REINHARD0 else l * (mul * l + 1.0) / (1.0 + l)
        if luminance_only:
            sf = scale(key * c[..., 1:2] / lw[1])
            return sf * np.where(ok, c, MAUVE)
        sf = scale(key * c / lw)
        if tonemap == REINHARD0:
            return sf * np.where(ok, c, MAUVE)
        o = sf * c
        return np.where(np.isfinite(o).all(-1)[..., None], o, MAUVE)


def oetf(v, params):
    """The OETF and its derivative."""
    knee, slope, a, g, b = params
    with np.errstate(all="ignore"):
        below = v < knee
        vp = np.where(below, 1.0, v)
        return np.where(below, slope * v, a * vp ** g - b), np.where(below, slope, a * g * vp ** (g - 1.0))


def matrix_of(colorspace):
    return M2020 if colorspace == REC2020 else M709      # sRGB and Rec709 share the Rec709 primaries (tonemap/mod.rs:243-296)


def oetf_of(colorspace):
    return OETF_SRGB if colorspace == SRGB else OETF_REC709


class Output:
    """One output_film case read in f64: lw, xyz (tonemapped), rgb (linear, before the OETF), s (OETF * 255), codes (the
    8-bit values, [..., 3]), err (E of check_output per code), linear and linear_err (the EXR's linear RGB and its bound)."""


def output_film(film, tonemap=CLAMP, luminance_only=True, exposure=0.0, key_value=0.18, white_point=1.0, colorspace=SRGB,
                factor=1.0, lw=None, matrix=None, oetf_params=None, quantize="ceil"):
    """output_film (src/renderer/mod.rs:24-80).  lw / matrix / oetf_params / quantize replace a piece of the reading for the
    sensitivity tests."""
    film = np.asarray(film, F32)
    r = Output()
    if lw is None:
        lw = np.ones(3) if tonemap == CLAMP else log_average(film, tonemap, luminance_only, factor)
    r.lw = lw
    r.xyz = map_pixels(film, tonemap, luminance_only, exposure, key_value, white_point, factor, lw)
    m = matrix_of(colorspace) if matrix is None else matrix
    with np.errstate(all="ignore"):
        r.rgb = r.xyz @ m.T
        mag = np.abs(r.xyz) @ np.abs(m).T                        # sum_j |m_ij o_j|
        enc, slope = oetf(r.rgb, oetf_of(colorspace) if oetf_params is None else oetf_params)
        r.s = enc * 255.0                                         # (r * 255.0).ceil().clamp(0.0, 255.0) as u8, tonemap/mod.rs:325-330
        q = np.ceil(r.s) if quantize == "ceil" else np.floor(r.s + 0.5)
        r.codes = np.where(np.isnan(r.s), 0, np.clip(q, 0, 255)).astype(np.uint8)   # NaN as u8 is 0
        r.err = 255.0 * np.abs(slope) * EPS * (mag + np.abs(r.rgb))
        fc = film[..., :3].astype(np.float64) * float(F32(factor))
        r.linear = fc @ m.T                                       # (factor * film.at(x, y)) in S primaries, tonemap/mod.rs:239-242
        r.linear_err = EPS * (np.abs(fc) @ np.abs(m).T + np.abs(r.linear))
    return r


def check_output(ref, rgba, linear=None):
    """Violations of the error model, by kind (all zero = the implementation agrees with `ref`):
      codes   - an 8-bit code other than ceil(s) clamped to 0..255, unless it differs by exactly one and s lies within E of
                the integer between them: the code lies in [ceil(s - E), ceil(s + E)] and within one of ceil(s).  The 0 and
                255 clamps and NaN -> 0 are exact (a MAUVE decision that differs moves a code by far more than one);
      alpha   - an alpha byte other than 255;
      linear  - linear RGB further than linear_err from the reading, or a different NaN / inf pattern."""
    rgba = np.asarray(rgba)
    nan = np.isnan(ref.s)
    with np.errstate(invalid="ignore"):
        c = np.ceil(ref.s)
        lo = np.clip(np.maximum(np.ceil(ref.s - ref.err), c - 1), 0, 255)
        hi = np.clip(np.minimum(np.ceil(ref.s + ref.err), c + 1), 0, 255)
    code = rgba[..., :3].astype(np.float64)
    bad = np.where(nan, code != 0, ~((code >= lo) & (code <= hi)))
    out = {"codes": int(bad.sum()), "alpha": int((rgba[..., 3] != 255).sum())}
    if linear is not None:
        lin = np.asarray(linear, np.float64)
        fin = np.isfinite(ref.linear)
        with np.errstate(invalid="ignore"):
            far = fin & ~(np.abs(lin - ref.linear) <= ref.linear_err)
        pattern = ~fin & ~((np.isnan(lin) & np.isnan(ref.linear)) | (lin == ref.linear))
        out["linear"] = int(far.sum() + pattern.sum())
    return out


def assert_output(ref, rgba, linear=None):
    v = check_output(ref, rgba, linear)
    assert not any(v.values()), v


def non_degenerate(rgba):
    """(distinct 8-bit values among R, G, B; fraction of pixels with some non-zero channel)."""
    c = np.asarray(rgba)[..., :3]
    return np.unique(c).size, float((c.reshape(-1, 3) != 0).any(-1).mean())


# ---- compare_exr --------------------------------------------------------------------------------------------------
# colorgrad::viridis() (a Cargo dependency, not in the reference tree): the uniform B-spline ("basis" interpolation) through
# the preset's nine sRGB keys, t clamped to [0, 1] (a NaN t taken as 0).
VIRIDIS = np.array([[0x44, 0x01, 0x54], [0x48, 0x27, 0x77], [0x3f, 0x4a, 0x8a], [0x31, 0x67, 0x8e], [0x26, 0x83, 0x8f],
                    [0x1f, 0x9d, 0x8a], [0x6c, 0xce, 0x5a], [0xb6, 0xde, 0x2b], [0xfe, 0xe8, 0x25]], np.float64) / 255.0


def viridis(t):
    t = np.asarray(t, np.float64)
    t = np.minimum(np.where(t >= 0.0, t, 0.0), 1.0)
    n = len(VIRIDIS)
    i = np.where(t >= 1.0, n - 2, np.floor(t * (n - 1))).astype(np.int64)
    u = (t - i / (n - 1)) * (n - 1)
    k = np.concatenate([2 * VIRIDIS[:1] - VIRIDIS[1:2], VIRIDIS, 2 * VIRIDIS[-1:] - VIRIDIS[-2:-1]])   # the end points reflected
    v0, v1, v2, v3 = k[i], k[i + 1], k[i + 2], k[i + 3]
    u = u[..., None]
    b = ((1 - u) ** 3 * v0 + (3 * u ** 3 - 6 * u ** 2 + 4) * v1 + (-3 * u ** 3 + 3 * u ** 2 + 3 * u + 1) * v2 + u ** 3 * v3) / 6.0
    return np.clip(b, 0.0, 1.0)


class Comparison:
    """out ([H, W, 4] f32; the RMSE mode's viridis colours as f64), value (the per-pixel scalar), and the statistics of
    pt_compare_stats: linf, mean_abs (per channel), rmse, pixel_min, pixel_max, nonfinite."""


def compare_films(image, truth, mode):
    """compare_exr.rs on raw [H, W, 4] f32 images.  Absolute: |a - b| per channel (:74-82).  RMSE: sqrt of the f32x4
    reduce_sum of d * d (a pairwise sum) / 4, splat, fourth lane 0 (:93-104), then viridis((r - min) / (max - min)) in f32
    (:106-127).  Relative: |a - b| / b, 0 where that is not finite (:150-161).  The statistics skip pixels with a non-finite
    channel in either image: per-channel max and mean of |d|, sqrt(sum d^2 / (4 good)), the min and max of the per-pixel value
    (the RMSE, or the largest channel of the other modes), and the number skipped; all zero when nothing is left."""
    a, b = np.asarray(image, F32), np.asarray(truth, F32)
    r = Comparison()
    with np.errstate(all="ignore"):
        d = a - b
        if mode == RMSE:
            q = d * d
            v = np.sqrt(((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) / F32(4.0))
            r.out = np.stack([v, v, v, np.zeros_like(v)], -1)
            r.value = v
        else:
            o = np.abs(d)
            if mode == RELATIVE:
                o = o / b
                o = np.where(np.isfinite(o), o, F32(0.0))
            r.out = o
            r.value = np.fmax(np.fmax(o[..., 0], o[..., 1]), np.fmax(o[..., 2], o[..., 3]))
    good = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    g = int(good.sum())
    dg = np.abs(d[good].astype(np.float64))
    r.nonfinite = int(good.size - g)
    r.linf = dg.max(axis=0) if g else np.zeros(4)
    r.mean_abs = np.array([math.fsum(dg[:, c]) for c in range(4)]) / g if g else np.zeros(4)     # exact sums, rounded once
    r.rmse = math.sqrt(math.fsum((dg * dg).ravel()) / (4.0 * g)) if g else 0.0
    r.pixel_min = F32(r.value[good].min()) if g else F32(0.0)
    r.pixel_max = F32(r.value[good].max()) if g else F32(0.0)
    if mode == RMSE:
        with np.errstate(all="ignore"):
            t = (r.value - r.pixel_min) / (r.pixel_max - r.pixel_min)      # f32, then as f64
        r.colours = np.concatenate([viridis(t.astype(np.float64)), np.ones(t.shape + (1,))], -1)
    return r
