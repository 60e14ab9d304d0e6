// pt_denoise_spectral_rules.h — the rules of the joint filter of the film and its wavelength bins (pt_denoise_spectral of include/pt_spectral.h, DESIGN.md
// section 14, "Denoising the bins") as PT_HD functions that the engine's kernels (pt_denoise.hip) and the host emulation of the tests
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
// request, so after any edit of this header re-run tools/resource_usage.py pt_denoise.hip: scratch 0 and no spills is the check.  (Undefined at the end of
// the header.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_UNROLL _Pragma("unroll")
#else
#define DN_UNROLL
#endif

namespace ptd {

// ---- prepare: a pixel with a bin that is not finite is dead, whatever its film holds.  `bin`: float (uint32_t b), the pixel's bins
template <class Bin>
PT_HD uint32_t dn_spectral_dead(uint32_t bins, Bin&& bin) {
    uint32_t dead = 0u;
    for (uint32_t b = 0; b < bins; ++b) dead |= pt_isfinite(bin(b)) ? 0u : (uint32_t)DN_DEAD;
    return dead;
}

// ---- one pass
// The colour, and the taps the bins are averaged with, are dn_gather_pixel_taps' (pt_denoise_rules.h): the film filter's gather with its taps kept.
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
