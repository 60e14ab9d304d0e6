// pt_denoise_spectral_rules.h — the rules of the joint filter of the film and its wavelength bins (pt_denoise_spectral of include/pt_spectral.h, DESIGN.md
// section 14, "Denoising the bins") as PT_HD functions that the engine's kernels (pt_denoise_spectral.hip) and the host emulation of the tests
// (tests/host_emulation/ptemu_denoise_spectral.cpp) compile from the same text.  It rests on pt_denoise_rules.h: a pass's taps and their weights are
// dn_gather_pixel's, computed once per pixel and kept (DnTaps), and every bin plane is averaged with them.  All arithmetic is f32, without contraction, in
// the order written.
//
// The source `S` of a pass is pt_denoise_rules.h's (flags, color, geo, tent) plus
//   float S::bin(uint32_t b, int x, int y)   s_b,i of an in-film pixel
#ifndef PT_DENOISE_SPECTRAL_RULES_H
#define PT_DENOISE_SPECTRAL_RULES_H
#include "pt_denoise_rules.h"

// Full unrolling on the device is what keeps DnTaps::w in registers: a loop left rolled indexes it at run time and sends it to scratch.  The pragma is a
// request, so after any edit of this header re-run tools/resource_usage.py pt_denoise_spectral.hip: scratch 0 and no spills is the check.  (Undefined at the
// end of the header.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_UNROLL _Pragma("unroll")
#else
#define DN_UNROLL
#endif

namespace ptd {

enum { DN_TAPS = 25, DN_CENTRE_TAP = 12 };

// the taps of one pixel in one pass: tap t = (dy + 2) * 5 + (dx + 2) is taken when bit t of `mask` is set, with the weight w[t] (0.0f for a tap not
// taken: never used); sw = the sum of the taken weights in tap order.  A dead pixel takes no tap (mask 0); a live one always takes its centre.
struct DnTaps { float w[DN_TAPS]; float sw; uint32_t mask; };

// ---- prepare: a pixel with a bin that is not finite is dead, whatever its film holds.  `bin`: float (uint32_t b), the pixel's bins
template <class Bin>
PT_HD uint32_t dn_spectral_dead(uint32_t bins, Bin&& bin) {
    uint32_t dead = 0u;
    for (uint32_t b = 0; b < bins; ++b) dead |= pt_isfinite(bin(b)) ? 0u : (uint32_t)DN_DEAD;
    return dead;
}

// ---- one pass
// dn_gather_pixel with its taps kept: the same taps in the same order, the same weights, the same sums — the colour it returns is dn_gather_pixel's bit
// for bit.  It is a second text of dn_gather_pixel (pt_denoise_rules.h), which pt_denoise_film's kernel keeps compiling as it stands: A CHANGE TO EITHER MUST
// BE MADE IN BOTH, and tests/test_denoise_spectral.py (the film and variance of the joint filter against ptemu_denoise_film's) is what notices when it was not.
// Both loops have constant bounds and are unrolled on the device, so that every index into T->w is static and the weights stay in registers.
template <class S>
PT_HD DnColor dn_gather_pixel_taps(const S& src, const DnParams& P, int step, int x, int y, float grad_x, float grad_y, DnTaps* T) {
    const uint32_t fp = src.flags(x, y);
    const DnColor cp = src.color(x, y);
    T->mask = 0u; T->sw = 0.0f;
    DN_UNROLL
    for (int t = 0; t < DN_TAPS; ++t) T->w[t] = 0.0f;
    if (fp & DN_DEAD) return cp;
    const DnGeo gp = src.geo(x, y);
    const float tp = src.tent(x, y);
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
    uint32_t mask = 0u;
    DN_UNROLL
    for (int dy = -2; dy <= 2; ++dy) {
        DN_UNROLL
        for (int dx = -2; dx <= 2; ++dx) {
            const int t = (dy + 2) * 5 + (dx + 2);
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
            T->w[t] = w;
            mask |= 1u << t;
            sw = sw + w;
            sx = sx + w * cq.x; sy = sy + w * cq.y; sz = sz + w * cq.z;
            sv = sv + (w * w) * cq.v;
        }
    }
    T->mask = mask; T->sw = sw;
    DnColor o;
    o.x = sx / sw; o.y = sy / sw; o.z = sz / sw; o.v = sv / (sw * sw);
    return o;
}

// s_b,i+1(p) for the N bins b0 .. b0+N-1 of a live pixel: sb = 0.0f, then sb = sb + w_q * s_b,i(q) over the taken taps in tap order, then sb / sw.
// A tap that is not taken adds nothing: its sum is selected away, not multiplied by 0, and the value read in its place is p's own (inside the film, and
// finite since p is live) — a tap outside the film is never read, a dead neighbour's bins never enter a sum.
template <int N, class S>
PT_HD void dn_gather_bins(const S& src, int step, int x, int y, const DnTaps& T, uint32_t b0, float* out) {
    float sb[N];
    DN_UNROLL
    for (int k = 0; k < N; ++k) sb[k] = 0.0f;
    DN_UNROLL
    for (int dy = -2; dy <= 2; ++dy) {
        DN_UNROLL
        for (int dx = -2; dx <= 2; ++dx) {
            const int t = (dy + 2) * 5 + (dx + 2);
            const bool taken = ((T.mask >> t) & 1u) != 0u;
            const int qx = taken ? x + dx * step : x, qy = taken ? y + dy * step : y;
            DN_UNROLL
            for (int k = 0; k < N; ++k) {
                const float s = src.bin(b0 + (uint32_t)k, qx, qy);
                const float added = sb[k] + T.w[t] * s;
                sb[k] = taken ? added : sb[k];
            }
        }
    }
    DN_UNROLL
    for (int k = 0; k < N; ++k) out[k] = sb[k] / T.sw;
}

// every bin of one pixel: a dead pixel keeps its own; a live one runs the taps once per chunk of DN_BIN_CHUNK bins, and the remainder as chunks of 4, 2
// and 1.  `store`: void (uint32_t b, float value)
enum { DN_BIN_CHUNK = 8 };
template <int N, class S, class Store>
PT_HD void dn_gather_bins_store(const S& src, int step, int x, int y, const DnTaps& T, uint32_t b0, Store&& store) {
    float o[N];
    dn_gather_bins<N>(src, step, x, y, T, b0, o);
    DN_UNROLL
    for (int k = 0; k < N; ++k) store(b0 + (uint32_t)k, o[k]);
}
template <class S, class Store>
PT_HD void dn_gather_pixel_bins(const S& src, int step, int x, int y, const DnTaps& T, uint32_t bins, Store&& store) {
    if (T.mask == 0u) {
        for (uint32_t b = 0; b < bins; ++b) store(b, src.bin(b, x, y));
        return;
    }
    uint32_t b = 0;
    for (; b + (uint32_t)DN_BIN_CHUNK <= bins; b += (uint32_t)DN_BIN_CHUNK) dn_gather_bins_store<DN_BIN_CHUNK>(src, step, x, y, T, b, store);
    if ((bins - b) & 4u) { dn_gather_bins_store<4>(src, step, x, y, T, b, store); b += 4u; }
    if ((bins - b) & 2u) { dn_gather_bins_store<2>(src, step, x, y, T, b, store); b += 2u; }
    if ((bins - b) & 1u) { dn_gather_bins_store<1>(src, step, x, y, T, b, store); }
}

}  // namespace ptd
#undef DN_UNROLL
#endif
