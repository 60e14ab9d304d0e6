// pt_denoise_rules.h — the rules of the film denoiser (include/pt_denoise.h) as PT_HD functions that the engine's kernels
// (pt_denoise.hip) and the host emulation of the tests (tests/host_emulation/ptemu_denoise.cpp) compile from the same text: the guide fold, the
// prepared inputs (variance of the mean from the f64 statistics, dead mask, unit normals, depth gradient), the 3x3 variance tent and the 25-tap
// edge-avoiding gather of one a-trous pass.  All arithmetic is f32 unless a double is written, evaluated without contraction and in the order
// written here; a numpy restatement (tests/test_denoise.py) gets every result bit for bit.
//
// The pixel functions are templates over a source `S` of the pass's inputs, so that a kernel may hand them global memory or a tile it staged:
//   uint32_t S::flags(int x, int y)   DN_DEAD | DN_SKY of an in-film pixel
//   DnColor  S::color(int x, int y)   c_i (x, y, z) and v_i (v)
//   DnGeo    S::geo(int x, int y)     unit normal (0 for sky) and depth
//   float    S::tent(int x, int y)    the pass's filtered variance (gather only)
#ifndef PT_DENOISE_RULES_H
#define PT_DENOISE_RULES_H
#include <stdint.h>

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

// c_{i+1}(p), v_{i+1}(p): the 25 taps in dy-outer, dx-inner order; a tap outside the film, dead, or sky against surface is skipped; a dead p is
// copied through
template <class S>
PT_HD DnColor dn_gather_pixel(const S& src, const DnParams& P, int step, int x, int y, float grad_x, float grad_y) {
    const uint32_t fp = src.flags(x, y);
    const DnColor cp = src.color(x, y);
    if (fp & DN_DEAD) return cp;
    const DnGeo gp = src.geo(x, y);
    const float tp = src.tent(x, y);
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
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
            sw = sw + w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            sv = sv + (w * w) * cq.v;
        }
    DnColor o;
    o.x = sx / sw; o.y = sy / sw; o.z = sz / sw; o.v = sv / (sw * sw);
    return o;
}

}  // namespace ptd
#endif
