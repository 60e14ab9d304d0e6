// pt_denoise_resident_rules.h — the rules of the joint filter's resident form (pt_denoise_resident of include/pt_resident.h, DESIGN.md section 14, "The
// resident filter") as PT_HD functions that the engine's kernels (pt_denoise.hip) and the host emulation of the tests
// (tests/host_emulation/ptemu_denoise_resident.cpp) compile from the same text.  It rests on pt_denoise_spectral_rules.h (the taps and the per-bin
// arithmetic of a pass) and pt_denoise_spectral_albedo_rules.h (the bins' division and multiplication), whose text stays: what is new here is where a bin
// lies between the passes.  All arithmetic is f32, without contraction, in the order written; no operation couples two bins, so a bin's bits are the
// plane-major filter's.
//
// The layout.  The ping-pong buffers of the passes hold Q = dn_quad_count(B) planes of quads: the quad at dn_quad_index(q, plane, pixel) holds the bins
// 4q .. 4q+3 of that pixel (plane = width x height, the index a size_t).  The bins B .. 4Q-1 of the last quad are pads: 0.0f from dn_bins_to_quads_pixel on,
// carried through the passes (0 + w * 0, 0 / sw), never tested and never read out.
//
// The source `S` of a pass is pt_denoise_rules.h's (flags, color, geo, tent) plus
//   DnQuad S::bin4(uint32_t q, int x, int y)   the quad q of an in-film pixel
#ifndef PT_DENOISE_RESIDENT_RULES_H
#define PT_DENOISE_RESIDENT_RULES_H
#include "pt_denoise_spectral_rules.h"
#include "pt_denoise_spectral_albedo_rules.h"

// (as in pt_denoise_spectral_rules.h: full unrolling on the device keeps DnTaps::w and a chunk's sums in registers — after an edit re-run
// tools/resource_usage.py pt_denoise.hip: scratch 0 and no spills is the check.  Undefined at the end of the header.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_UNROLL _Pragma("unroll")
#else
#define DN_UNROLL
#endif

namespace ptd {

// four bins of one pixel: a native vector of both compilers, so that a quad moves as one 16-byte load or store; the arithmetic is per element
typedef float DnQuad __attribute__((vector_size(16)));

// ---- the index rule
PT_HD uint32_t dn_quad_count(uint32_t bins) { return (bins + 3u) / 4u; }
PT_HD size_t dn_quad_index(uint32_t q, size_t plane, size_t pixel) { return (size_t)q * plane + pixel; }
PT_HD uint32_t dn_quad_of_bin(uint32_t b) { return b >> 2; }
PT_HD uint32_t dn_quad_lane_of_bin(uint32_t b) { return b & 3u; }

// ---- before the passes: one pixel's plane-major bins into quads, with dn_bins_demodulate_pixel's division and dead test per bin, in bin order.  The
// pixel is dead when `flags` says so or when a bin is not finite before or after the division; a dead pixel keeps the bins it came with.  Returns DN_DEAD or 0.
//   `raw`: float (uint32_t b), s_b    `alb`: float (uint32_t b), A_b (1.0f where there is no per-bin albedo)    `store`: void (uint32_t q, DnQuad)
template <class Raw, class Alb, class Store>
PT_HD uint32_t dn_bins_to_quads_pixel(uint32_t bins, uint32_t flags, Raw&& raw, Alb&& alb, Store&& store) {
    uint32_t dead = flags & (uint32_t)DN_DEAD;
    const uint32_t quads = dn_quad_count(bins);
    for (uint32_t q = 0; q < quads; ++q) {
        DnQuad o;
        DN_UNROLL
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t b = 4u * q + j;
            float v = 0.0f;
            if (b < bins) {
                const float s = raw(b);
                v = s / dn_bin_divisor(alb(b));
                dead |= (pt_isfinite(s) && pt_isfinite(v)) ? 0u : (uint32_t)DN_DEAD;
            }
            o[j] = v;
        }
        store(q, o);
    }
    if (dead)
        for (uint32_t q = 0; q < quads; ++q) {
            DnQuad o;
            DN_UNROLL
            for (uint32_t j = 0; j < 4u; ++j) { const uint32_t b = 4u * q + j; o[j] = b < bins ? raw(b) : 0.0f; }
            store(q, o);
        }
    return dead;
}

// ---- after the last pass: one pixel's quads into plane-major bins, a live pixel's multiplied back (dn_bin_remodulate) where there is a per-bin albedo; a
// dead pixel keeps what the passes copied through: its input bits.
//   `quad`: DnQuad (uint32_t q)    `alb`: float (uint32_t b), read for a live pixel with HAS_A alone    `store`: void (uint32_t b, float)
template <bool HAS_A, class Quad, class Alb, class Store>
PT_HD void dn_quads_to_bins_pixel(uint32_t bins, uint32_t flags, Quad&& quad, Alb&& alb, Store&& store) {
    const bool multiply = HAS_A && !(flags & (uint32_t)DN_DEAD);
    const uint32_t quads = dn_quad_count(bins);
    for (uint32_t q = 0; q < quads; ++q) {
        const DnQuad s = quad(q);
        DN_UNROLL
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t b = 4u * q + j;
            if (b < bins) store(b, multiply ? dn_bin_remodulate(s[j], alb(b)) : s[j]);
        }
    }
}

// ---- one pass: dn_gather_bins' arithmetic for the 4 NQ bins of the quads q0 .. q0+NQ-1 of a live pixel, per bin in the same order — sb = 0.0f, then
// sb = sb + w_q * s_b,i(q) over the taken taps in tap order, then sb / sw — with one read of a quad per tap where dn_gather_bins reads four planes.
template <int NQ, class S>
PT_HD void dn_gather_bins4(const S& src, int step, int x, int y, const DnTaps& T, uint32_t q0, DnQuad* out) {
    float sb[NQ][4];
    DN_UNROLL
    for (int k = 0; k < NQ; ++k) {
        DN_UNROLL
        for (int j = 0; j < 4; ++j) sb[k][j] = 0.0f;
    }
    DN_UNROLL
    for (int dy = -2; dy <= 2; ++dy) {
        DN_UNROLL
        for (int dx = -2; dx <= 2; ++dx) {
            const int t = (dy + 2) * 5 + (dx + 2);
            const bool taken = ((T.mask >> t) & 1u) != 0u;
            const int qx = taken ? x + dx * step : x, qy = taken ? y + dy * step : y;
            DN_UNROLL
            for (int k = 0; k < NQ; ++k) {
                const DnQuad s = src.bin4(q0 + (uint32_t)k, qx, qy);
                DN_UNROLL
                for (int j = 0; j < 4; ++j) {
                    const float added = sb[k][j] + T.w[t] * s[j];
                    sb[k][j] = taken ? added : sb[k][j];
                }
            }
        }
    }
    DN_UNROLL
    for (int k = 0; k < NQ; ++k) {
        DN_UNROLL
        for (int j = 0; j < 4; ++j) out[k][j] = sb[k][j] / T.sw;
    }
}

// every quad of one pixel: a dead pixel keeps its own; a live one runs the taps once per chunk of DN_QUAD_CHUNK quads (DN_BIN_CHUNK bins), and the
// remainder as one quad.  `store`: void (uint32_t q, DnQuad value)
enum { DN_QUAD_CHUNK = 2 };
template <int NQ, class S, class Store>
PT_HD void dn_gather_bins4_store(const S& src, int step, int x, int y, const DnTaps& T, uint32_t q0, Store&& store) {
    DnQuad o[NQ];
    dn_gather_bins4<NQ>(src, step, x, y, T, q0, o);
    DN_UNROLL
    for (int k = 0; k < NQ; ++k) store(q0 + (uint32_t)k, o[k]);
}
template <class S, class Store>
PT_HD void dn_gather_pixel_bins4(const S& src, int step, int x, int y, const DnTaps& T, uint32_t quads, Store&& store) {
    if (T.mask == 0u) {
        for (uint32_t q = 0; q < quads; ++q) store(q, src.bin4(q, x, y));
        return;
    }
    uint32_t q = 0;
    for (; q + (uint32_t)DN_QUAD_CHUNK <= quads; q += (uint32_t)DN_QUAD_CHUNK) dn_gather_bins4_store<DN_QUAD_CHUNK>(src, step, x, y, T, q, store);
    if ((quads - q) & 1u) dn_gather_bins4_store<1>(src, step, x, y, T, q, store);
}

}  // namespace ptd
#undef DN_UNROLL
#endif
