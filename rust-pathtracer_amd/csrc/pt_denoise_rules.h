// pt_denoise_rules.h — the rules of the film denoiser (include/pt_denoise.h) as PT_HD functions that the engine's kernels
// (pt_denoise.hip) and the host emulation of the tests (tests/host_emulation/ptemu_denoise.cpp, ptemu_denoise_albedo.cpp) compile from the same
// text: the guide fold, the prepared inputs (variance of the mean from the f64 statistics, dead mask, unit normals, depth gradient), the 3x3
// variance tent and the 25-tap edge-avoiding gather of one a-trous pass, and (last in the file) the albedo guide with the film's demodulation by
// it.  All arithmetic is f32 unless a double is written, evaluated without contraction and in the order written here; a numpy restatement
// (tests/test_denoise.py, tests/test_denoise_albedo.py) gets every result bit for bit.
//
// The pixel functions are templates over a source `S` of the pass's inputs, so that a kernel may hand them global memory or a tile it staged:
//   uint32_t S::flags(int x, int y)   DN_DEAD | DN_SKY of an in-film pixel
//   DnColor  S::color(int x, int y)   c_i (x, y, z) and v_i (v)
//   DnGeo    S::geo(int x, int y)     unit normal (0 for sky) and depth
//   float    S::tent(int x, int y)    the pass's filtered variance (gather only)
#ifndef PT_DENOISE_RULES_H
#define PT_DENOISE_RULES_H
#include <stdint.h>

#include "../../include/pt_api.h"
#include "../../include/pt_numerics.h"

namespace ptd {

enum { DN_DEAD = 1u, DN_SKY = 2u };
enum { DN_DEFAULT_ITERATIONS = 5, DN_MAX_ITERATIONS = 10, DN_DEFAULT_NORMAL_POWER_LOG2 = 7, DN_MAX_NORMAL_POWER_LOG2 = 10 };
#define DN_DEFAULT_SIGMA_LUMINANCE 4.0f
#define DN_DEFAULT_SIGMA_DEPTH 1.0f

struct DnColor { float x, y, z, v; };
struct DnGeo { float nx, ny, nz, z; };
struct DnGuideSum { float nx, ny, nz, z; uint32_t hits; };
struct DnParams { uint32_t width, height; float sigma_l, sigma_z; uint32_t normal_squarings; };

// ---- guides: N += hit.normal and Z += hit.t over the valid hits in sample order; G = (N / K, hits ? Z / hits : 0)
PT_HD void dn_guide_add(DnGuideSum* g, int valid, float t, float nx, float ny, float nz) {
    if (valid) { g->nx += nx; g->ny += ny; g->nz += nz; g->z += t; g->hits += 1u; }
}
PT_HD DnGeo dn_guide_finish(const DnGuideSum& g, uint32_t samples) {
    const float k = (float)samples;
    DnGeo o;
    o.nx = g.nx / k; o.ny = g.ny / k; o.nz = g.nz / k;
    o.z = g.hits ? g.z / (float)g.hits : 0.0f;
    return o;
}

// ---- prepared inputs
// the variance of the pixel's mean Y: max(n S2 - S1^2, 0) / (n n (n - 1)) in f64, rounded once (a NaN stays one: the pixel is dead)
PT_HD float dn_variance(uint32_t n, double s1, double s2) {
    const double nd = (double)n;
    double num = nd * s2 - s1 * s1;
    num = num < 0.0 ? 0.0 : num;
    return (float)(num / (nd * nd * (nd - 1.0)));
}
PT_HD uint32_t dn_dead(float x, float y, float z, float v) {
    return (pt_isfinite(x) && pt_isfinite(y) && pt_isfinite(z) && pt_isfinite(v)) ? 0u : (uint32_t)DN_DEAD;
}
// the unit normal of a guide pixel; |N| == 0 is sky (unit normal 0)
PT_HD DnGeo dn_unit(float nx, float ny, float nz, float z, uint32_t* sky) {
    const float len = pt_sqrt((nx * nx + ny * ny) + nz * nz);
    const bool is_sky = len == 0.0f;
    DnGeo o;
    o.nx = is_sky ? 0.0f : nx / len; o.ny = is_sky ? 0.0f : ny / len; o.nz = is_sky ? 0.0f : nz / len; o.z = z;
    *sky = is_sky ? (uint32_t)DN_SKY : 0u;
    return o;
}
// one component of the depth gradient at position i of a line of n depths: central difference, one-sided at the ends, 0 for a line of one
PT_HD float dn_gradient(float z_before, float z_here, float z_after, uint32_t i, uint32_t n) {
    if (n < 2u) return 0.0f;
    if (i == 0u) return z_after - z_here;
    if (i + 1u == n) return z_here - z_before;
    return (z_after - z_before) * 0.5f;
}

// ---- one pass
// the 3x3 tent (2 - |dx|)(2 - |dy|) average of v over the live in-film neighbours, dy outer, dx inner; 0 for a dead pixel (never read)
template <class S>
PT_HD float dn_tent_pixel(const S& src, const DnParams& P, int x, int y) {
    if (src.flags(x, y) & DN_DEAD) return 0.0f;
    float sum = 0.0f, wsum = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)P.width || qy >= (int)P.height) continue;
            if (src.flags(qx, qy) & DN_DEAD) continue;
            const float g = (float)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
            sum = sum + g * src.color(qx, qy).v;
            wsum = wsum + g;
        }
    return sum / wsum;
}

PT_HD float dn_kernel(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// the edge-stopping weight of the tap q = p + step (dx, dy), (dx, dy) != (0, 0), both live and both sky or both surface: kernel x geometry x luminance
PT_HD float dn_tap_weight(const DnParams& P, int dx, int dy, int step, uint32_t sky, const DnGeo& gp, float grad_x, float grad_y, float yp, float tent_p,
                          const DnGeo& gq, float yq, float tent_q) {
    float e = 1.0f;
    if (!sky) {
        float d = (gp.nx * gq.nx + gp.ny * gq.ny) + gp.nz * gq.nz;
        d = d > 0.0f ? d : 0.0f;
        for (uint32_t k = 0; k < P.normal_squarings; ++k) d = d * d;
        const float fx = (float)(dx * step), fy = (float)(dy * step);
        const float expected = pt_abs(grad_x * fx + grad_y * fy);
        const float den = (P.sigma_z * expected + 1e-3f * pt_abs(gp.z)) + 1e-30f;
        e = d * pt_exp(-pt_min(pt_abs(gp.z - gq.z) / den, 80.0f));
    }
    const float l = pt_exp(-pt_min(pt_abs(yp - yq) / (P.sigma_l * pt_sqrt(tent_p + tent_q) + 1e-20f), 80.0f));
    return ((dn_kernel(dx) * dn_kernel(dy)) * e) * l;
}

enum { DN_TAPS = 25, DN_CENTRE_TAP = 12 };

// the taps of one pixel in one pass, for the filters that average more planes with them (pt_denoise_spectral_rules.h): tap t = (dy + 2) * 5 + (dx + 2) is
// taken when bit t of `mask` is set, with the weight w[t] (0.0f for a tap not taken: never used); sw = the sum of the taken weights in tap order.  A dead
// pixel takes no tap (mask 0); a live one always takes its centre.
struct DnTaps { float w[DN_TAPS]; float sw; uint32_t mask; };

// c_{i+1}(p), v_{i+1}(p): the 25 taps in dy-outer, dx-inner order; a tap outside the film, dead, or sky against surface is skipped; a dead p is
// copied through.  This is the one text of the gather: dn_gather_pixel, below, is it with KEEP false (T is not looked at); with KEEP, the default, the
// taps are also recorded in *T, and the colour is the same bit for bit.  With KEEP both loops are unrolled on the device, so that every index into T->w
// is static and the weights stay in registers (a loop left rolled sends them to scratch); without it the loops stay rolled, as the compiler leaves them:
// a tap is some 200 instructions.  The pragma is a request, so after any edit of this function re-run tools/resource_usage.py pt_denoise.hip: scratch 0
// and no spills in k_dn_gather_spectral is the check.
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_UNROLL_TAPS _Pragma("clang loop unroll_count(KEEP ? 5 : 1)")   /* (KEEP: the template argument below) */
#else
#define DN_UNROLL_TAPS
#endif
template <bool KEEP = true, class S>
PT_HD DnColor dn_gather_pixel_taps(const S& src, const DnParams& P, int step, int x, int y, float grad_x, float grad_y, DnTaps* T) {
    const uint32_t fp = src.flags(x, y);
    const DnColor cp = src.color(x, y);
    if constexpr (KEEP) {
        T->mask = 0u; T->sw = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int t = 0; t < DN_TAPS; ++t) T->w[t] = 0.0f;
    }
    if (fp & DN_DEAD) return cp;
    const DnGeo gp = src.geo(x, y);
    const float tp = src.tent(x, y);
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
    [[maybe_unused]] uint32_t mask = 0u;
    DN_UNROLL_TAPS
    for (int dy = -2; dy <= 2; ++dy) {
        DN_UNROLL_TAPS
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step, qy = y + dy * step;
            if (qx < 0 || qy < 0 || qx >= (int)P.width || qy >= (int)P.height) continue;
            float w;
            DnColor cq;
            if (dx == 0 && dy == 0) {
                w = dn_kernel(0) * dn_kernel(0);
                cq = cp;
            } else {
                const uint32_t fq = src.flags(qx, qy);
                if ((fq & DN_DEAD) || ((fq ^ fp) & DN_SKY)) continue;
                cq = src.color(qx, qy);
                w = dn_tap_weight(P, dx, dy, step, fp & DN_SKY, gp, grad_x, grad_y, cp.y, tp, src.geo(qx, qy), cq.y, src.tent(qx, qy));
            }
            if constexpr (KEEP) {
                const int t = (dy + 2) * 5 + (dx + 2);
                T->w[t] = w;
                mask |= 1u << t;
            }
            sw = sw + w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            sv = sv + (w * w) * cq.v;
        }
    }
    if constexpr (KEEP) { T->mask = mask; T->sw = sw; }
    DnColor o;
    o.x = sx / sw; o.y = sy / sw; o.z = sz / sw; o.v = sv / (sw * sw);
    return o;
}
#undef DN_UNROLL_TAPS
template <class S>
PT_HD DnColor dn_gather_pixel(const S& src, const DnParams& P, int step, int x, int y, float grad_x, float grad_y) {
    return dn_gather_pixel_taps<false>(src, P, step, x, y, grad_x, grad_y, nullptr);
}

// ---- albedo: the first-hit reflectance of a Lambertian surface as XYZ factors, and the film divided by it before the passes
// The basis: DN_ALBEDO_WAVELENGTHS wavelengths at the centres of equal parts of the render's range, each with its colour-matching weights
// w[c][j] = xyz_bar(lambda_j x 10) (the form k_accumulate uses) and norm[c] = sum_j w[c][j], j ascending.  `X`: void (float angstrom, float*, float*, float*).
enum { DN_ALBEDO_WAVELENGTHS = 16 };
#define DN_ALBEDO_FLOOR 1e-3f
struct DnAlbedoBasis { float lambda[DN_ALBEDO_WAVELENGTHS]; float w[3][DN_ALBEDO_WAVELENGTHS]; float norm[3]; };
struct DnAlbedo { float x, y, z; };
struct DnTexel { uint32_t kind; float t0, t1, t2, t3; };   // a layer's texel at one (u, v): PT_TEXTURE1 holds t0 alone
struct DnLayerCurves { float c0, c1, c2, c3; };            // a layer's curves at one wavelength (layer_curves of pt_device.h)

PT_HD float dn_albedo_lambda(float lo, float hi, int j) { return lo + ((float)j + 0.5f) * ((hi - lo) / 16.0f); }
template <class X>
PT_HD void dn_albedo_basis(float lo, float hi, const X& xyz_bar_of, DnAlbedoBasis* B) {
    for (int j = 0; j < DN_ALBEDO_WAVELENGTHS; ++j) {
        B->lambda[j] = dn_albedo_lambda(lo, hi, j);
        xyz_bar_of(B->lambda[j] * 10.0f, &B->w[0][j], &B->w[1][j], &B->w[2][j]);
    }
    for (int c = 0; c < 3; ++c) {
        float s = 0.0f;
        for (int j = 0; j < DN_ALBEDO_WAVELENGTHS; ++j) s = s + B->w[c][j];
        B->norm[c] = s;
    }
}

// whether a hit has a material record to look at: valid, not the camera's own tag, the index inside the scene's materials
PT_HD bool dn_albedo_has_record(int valid, uint32_t material_id, uint32_t material_count) {
    return valid && PT_MATERIAL_TAG(material_id) != (uint32_t)PT_TAG_CAMERA && PT_MATERIAL_INDEX(material_id) < material_count;
}
// the texel(s) of the layer record at word `l` of the blob `w` (pt_blob.h: kind, four curves, width, height, texel offset) that layer_eval reads at (u, v)
PT_HD DnTexel dn_albedo_texel(const uint32_t* w, const float* tex, uint32_t l, float u, float v) {
    const uint32_t kind = w[l], tw = w[l + 5], th = w[l + 6], toff = w[l + 7];
    const float cu = pt_clamp(u, 0.0f, 1.0f - PT_F32_EPSILON), cv = pt_clamp(v, 0.0f, 1.0f - PT_F32_EPSILON);
    uint32_t x = (uint32_t)(cu * (float)tw), y = (uint32_t)(cv * (float)th);
    x = x < tw ? x : tw - 1u; y = y < th ? y : th - 1u;   // (never taken for a (u, v) in [0, 1]: no read leaves the texture whatever the hit record holds)
    const uint32_t idx = y * tw + x;
    DnTexel t;
    t.kind = kind; t.t1 = t.t2 = t.t3 = 0.0f;
    if (kind == (uint32_t)PT_TEXTURE1) { t.t0 = tex[toff + idx]; return t; }
    const float* p = tex + toff + 4u * idx;
    t.t0 = p[0]; t.t1 = p[1]; t.t2 = p[2]; t.t3 = p[3];
    return t;
}
// layer_eval's value from the texel and the curves
PT_HD float dn_layer_value(const DnTexel& t, const DnLayerCurves& c) {
    if (t.kind == (uint32_t)PT_TEXTURE1) return c.c0 * t.t0;
    const float e0 = c.c0 * t.t0, e1 = c.c1 * t.t1;
    const float e2 = c.c2 * t.t2, e3 = c.c3 * t.t3;
    return (e0 + e1) + (e2 + e3);
}
// a Lambertian hit's albedo: rho_j = min(texstack_eval(lambda_j, u, v), 1) — the bits material_prepare puts into its reflectance — folded over the basis.
// The texels depend on (u, v) only: a layer's are fetched once for the 16 wavelengths.  `T`: the hit's texture stack,
//   uint32_t T::layers()   DnTexel T::texel(uint32_t layer)   DnLayerCurves T::curves(uint32_t layer, int j)
template <class T>
PT_HD DnAlbedo dn_albedo_lambertian(const T& stack, const DnAlbedoBasis& B) {
    float energy[DN_ALBEDO_WAVELENGTHS];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < DN_ALBEDO_WAVELENGTHS; ++j) energy[j] = 0.0f;
    const uint32_t layers = stack.layers();
    for (uint32_t i = 0; i < layers; ++i) {
        const DnTexel t = stack.texel(i);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < DN_ALBEDO_WAVELENGTHS; ++j) energy[j] = energy[j] + dn_layer_value(t, stack.curves(i, j));
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < DN_ALBEDO_WAVELENGTHS; ++j) {
        const float rho = pt_min(energy[j], 1.0f);
        sx = sx + rho * B.w[0][j]; sy = sy + rho * B.w[1][j]; sz = sz + rho * B.w[2][j];
    }
    DnAlbedo a;
    a.x = B.norm[0] > 0.0f ? sx / B.norm[0] : 1.0f;
    a.y = B.norm[1] > 0.0f ? sy / B.norm[1] : 1.0f;
    a.z = B.norm[2] > 0.0f ? sz / B.norm[2] : 1.0f;
    return a;
}
// A(p) = (sum_k a_k) / K, the samples in order; everything but a valid Lambertian hit adds (1, 1, 1)
PT_HD void dn_albedo_add(DnAlbedo* s, const DnAlbedo& a) { s->x = s->x + a.x; s->y = s->y + a.y; s->z = s->z + a.z; }
PT_HD DnAlbedo dn_albedo_finish(const DnAlbedo& s, uint32_t samples) {
    const float k = (float)samples;
    DnAlbedo o;
    o.x = s.x / k; o.y = s.y / k; o.z = s.z / k;
    return o;
}

// c0' = c0 / d and v0' = v0 / d.Y^2 with d = max(A, DN_ALBEDO_FLOOR) per channel.  A pixel with a non-finite channel before or after the division is
// dead and keeps its own c0, v0: it is never read, and comes out as it went in.  (x / 1.0f and x * 1.0f are exact: an albedo of ones changes nothing.)
PT_HD DnColor dn_demodulate(const DnColor& c, const DnAlbedo& a, uint32_t* dead) {
    const float dx = pt_max(a.x, DN_ALBEDO_FLOOR), dy = pt_max(a.y, DN_ALBEDO_FLOOR), dz = pt_max(a.z, DN_ALBEDO_FLOOR);
    DnColor o;
    o.x = c.x / dx; o.y = c.y / dy; o.z = c.z / dz; o.v = c.v / (dy * dy);
    *dead = dn_dead(c.x, c.y, c.z, c.v) | dn_dead(o.x, o.y, o.z, o.v);
    return *dead ? c : o;
}
PT_HD DnColor dn_remodulate(const DnColor& c, const DnAlbedo& a, uint32_t flags) {
    if (flags & DN_DEAD) return c;
    const float dx = pt_max(a.x, DN_ALBEDO_FLOOR), dy = pt_max(a.y, DN_ALBEDO_FLOOR), dz = pt_max(a.z, DN_ALBEDO_FLOOR);
    DnColor o;
    o.x = c.x * dx; o.y = c.y * dy; o.z = c.z * dz; o.v = c.v * (dy * dy);
    return o;
}

}  // namespace ptd
#endif
