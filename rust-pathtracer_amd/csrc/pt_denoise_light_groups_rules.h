// pt_denoise_light_groups_rules.h — the rules of the joint filter over light-group films (pt_denoise_light_groups of include/pt_light_groups_denoise.h,
// DESIGN.md section 15, "Adaptive and denoised group films") as PT_HD functions that the engine's kernels (pt_denoise.hip) and the host emulation of the tests
// (tests/host_emulation/ptemu_denoise_light_groups.cpp) compile from the same text.  It rests on pt_denoise_spectral_rules.h (the taps of a pass, DnTaps),
// pt_denoise_spectral_albedo_rules.h (the divisor, the colour of a pixel dead through its planes alone) and pt_denoise_resident_rules.h (DnQuad, the index
// rule), whose text stays.  All arithmetic is f32, without contraction, in the order written; no operation couples two channels or two groups, so a channel's
// bits are those of the plane 3g + c in pt_denoise_spectral_albedo, which is the filter's definition.
//
// The layout is the group films' own between the passes too: group-major float4 films, the float4 of group g and pixel i at dn_quad_index(g, plane, i).
// x, y, z are filtered; w is 0 in every live pixel from the prepare on.  A dead pixel keeps all four floats it came with.
//
// The source `S` of a pass is pt_denoise_resident_rules.h's: (flags, color, geo, tent) plus
//   DnQuad S::bin4(uint32_t g, int x, int y)   the float4 of group g at an in-film pixel
#ifndef PT_DENOISE_LIGHT_GROUPS_RULES_H
#define PT_DENOISE_LIGHT_GROUPS_RULES_H
#include "pt_denoise_resident_rules.h"

// (as in pt_denoise_spectral_rules.h: full unrolling on the device keeps DnTaps::w and a chunk's sums in registers — after an edit re-run
// tools/resource_usage.py pt_denoise.hip: scratch 0 and no spills is the check.  Undefined at the end of the header.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_UNROLL _Pragma("unroll")
#else
#define DN_UNROLL
#endif

namespace ptd {

// ---- before the passes: one pixel's group films into the first ping-pong buffer.  Channel c of group g is divided by max(A_c, DN_ALBEDO_FLOOR) where HAS_A
// (dn_bins_demodulate_pixel's division with A[3g + c] = A_c); the pixel is dead when `flags` says so or when a channel of a group is not finite before or after
// the division; a dead pixel keeps the float4s it came with.  Returns DN_DEAD or 0.
//   `raw`: DnQuad (uint32_t g), group g's film pixel    `store`: void (uint32_t g, DnQuad), into a buffer that `raw` does not read
template <bool HAS_A, class Raw, class Store>
PT_HD uint32_t dn_groups_prepare_pixel(uint32_t groups, uint32_t flags, const DnAlbedo& a, Raw&& raw, Store&& store) {
    uint32_t dead = flags & (uint32_t)DN_DEAD;
    const float d[3] = {HAS_A ? dn_bin_divisor(a.x) : 1.0f, HAS_A ? dn_bin_divisor(a.y) : 1.0f, HAS_A ? dn_bin_divisor(a.z) : 1.0f};
    for (uint32_t g = 0; g < groups; ++g) {
        const DnQuad s = raw(g);
        DnQuad o;
        DN_UNROLL
        for (int c = 0; c < 3; ++c) {
            const float q = s[c] / d[c];   // (x / 1.0f is exact: without an albedo the planes are tested as they lie)
            dead |= (pt_isfinite(s[c]) && pt_isfinite(q)) ? 0u : (uint32_t)DN_DEAD;
            o[c] = q;
        }
        o[3] = 0.0f;
        store(g, o);
    }
    if (dead)
        for (uint32_t g = 0; g < groups; ++g) store(g, raw(g));
    return dead;
}

// ---- after the last pass: a live pixel's channels multiplied back (dn_bin_remodulate) where HAS_A, w = 0; a dead pixel keeps what the passes copied
// through: its input bits, w included.
template <bool HAS_A>
PT_HD DnQuad dn_groups_finish_pixel(uint32_t flags, const DnAlbedo& a, const DnQuad& s) {
    if (flags & (uint32_t)DN_DEAD) return s;
    DnQuad o;
    o[0] = HAS_A ? dn_bin_remodulate(s[0], a.x) : s[0];
    o[1] = HAS_A ? dn_bin_remodulate(s[1], a.y) : s[1];
    o[2] = HAS_A ? dn_bin_remodulate(s[2], a.z) : s[2];
    o[3] = 0.0f;
    return o;
}

// ---- one pass: pt_denoise_resident_rules.h's dn_gather_pixel_bins4 as it is, over `groups` quads: a group's float4 is a quad, x, y, z three of its bins, and
// w a fourth whose value is 0 in every live pixel (0.0f + w_q * 0.0f, then 0.0f / sw) and a dead pixel's own where it is copied through.  The source `S`
// names the group's float4 `bin4` for that text.  Summing three channels in a text of its own measured no faster, and slower at G = 8.

}  // namespace ptd
#undef DN_UNROLL
#endif
