// pt_denoise_spectral_albedo_rules.h — the rules of the per-bin albedo guide and of the joint filter that demodulates the bins by it
// (pt_render_guides_bin_albedo and pt_denoise_spectral_albedo of include/pt_spectral.h, DESIGN.md section 14, "Demodulating the bins") as PT_HD functions
// that the engine's kernels (pt_denoise_spectral_albedo.hip and pt_guides_chain.hip for the guide, pt_denoise.hip for the filter) and the host emulation
// of the tests (tests/host_emulation/ptemu_denoise_spectral_albedo.cpp) compile from the same text.  It rests on pt_denoise_rules.h (the albedo rule of
// one layer, the floor) and pt_denoise_spectral_rules.h (the passes, which are unchanged).  All arithmetic is f32, without contraction, in the order written.
#ifndef PT_DENOISE_SPECTRAL_ALBEDO_RULES_H
#define PT_DENOISE_SPECTRAL_ALBEDO_RULES_H
#include "pt_blob.h"
#include "pt_denoise_spectral_rules.h"

// (as in pt_denoise_spectral_rules.h: the chunk loops are unrolled on the device so that every index into a chunk's registers is static — after an edit
// re-run tools/resource_usage.py on pt_denoise_spectral_albedo.hip, pt_guides_chain.hip and pt_denoise.hip: scratch 0 is the check.  Undefined at the end of
// the header.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_UNROLL _Pragma("unroll")
#else
#define DN_UNROLL
#endif

namespace ptd {

// ---- the bins' wavelengths: pt_spectral_bin_centres' expression, lo + ((float)b + 0.5f) * w with w = (hi - lo) / (float)bins
PT_HD float dn_bin_width(float lo, float hi, uint32_t bins) { return (hi - lo) / (float)bins; }
PT_HD float dn_bin_centre(float lo, float w, uint32_t b) { return lo + ((float)b + 0.5f) * w; }

// ---- the per-bin albedo of one guide sample
// rho_b = min(texstack_eval(lambda_b, u, v), 1) for the N bins b0 .. b0+N-1 of a Lambertian hit, evaluated as dn_albedo_lambertian evaluates its 16
// wavelengths: energy_b from 0.0f plus dn_layer_value(texel_i, curves_i(lambda_b)) over the layers in order.  The texel of a layer depends on (u, v) alone,
// so every chunk sees the same one.  `T`: the hit's texture stack,
//   uint32_t T::layers()   DnTexel T::texel(uint32_t layer)   DnLayerCurves T::bin_curves(uint32_t layer, uint32_t b)
template <int N, class T>
PT_HD void dn_bin_albedo_rho(const T& stack, uint32_t b0, float* rho) {
    float energy[N];
    DN_UNROLL
    for (int k = 0; k < N; ++k) energy[k] = 0.0f;
    const uint32_t layers = stack.layers();
    for (uint32_t i = 0; i < layers; ++i) {
        const DnTexel t = stack.texel(i);
        DN_UNROLL
        for (int k = 0; k < N; ++k) energy[k] = energy[k] + dn_layer_value(t, stack.bin_curves(i, b0 + (uint32_t)k));
    }
    DN_UNROLL
    for (int k = 0; k < N; ++k) rho[k] = pt_min(energy[k], 1.0f);
}
// sum_b = sum_b + rho_b for N bins.  `sum`: float& (uint32_t b), the pixel's running sum of bin b
template <int N, class T, class Sum>
PT_HD void dn_bin_albedo_add_chunk(const T& stack, uint32_t b0, Sum&& sum) {
    float rho[N];
    dn_bin_albedo_rho<N>(stack, b0, rho);
    DN_UNROLL
    for (int k = 0; k < N; ++k) { float& s = sum(b0 + (uint32_t)k); s = s + rho[k]; }
}
// one guide sample into the sums of its pixel: `stack` null — a miss, or a hit that is not a Lambertian surface with a record — adds 1 to every bin; a
// Lambertian hit walks the bins in chunks of DN_BIN_CHUNK and the remainder as chunks of 4, 2 and 1, as dn_gather_pixel_bins does
template <class T, class Sum>
PT_HD void dn_bin_albedo_add(const T* stack, uint32_t bins, Sum&& sum) {
    if (!stack) {
        for (uint32_t b = 0; b < bins; ++b) { float& s = sum(b); s = s + 1.0f; }
        return;
    }
    uint32_t b = 0;
    for (; b + (uint32_t)DN_BIN_CHUNK <= bins; b += (uint32_t)DN_BIN_CHUNK) dn_bin_albedo_add_chunk<DN_BIN_CHUNK>(*stack, b, sum);
    if ((bins - b) & 4u) { dn_bin_albedo_add_chunk<4>(*stack, b, sum); b += 4u; }
    if ((bins - b) & 2u) { dn_bin_albedo_add_chunk<2>(*stack, b, sum); b += 2u; }
    if ((bins - b) & 1u) { dn_bin_albedo_add_chunk<1>(*stack, b, sum); }
}
// whether a hit is one whose texture stack is evaluated: k_guide_fold_albedo's test.  `w`: the scene blob; *ts = the word offset of the stack's record
PT_HD bool dn_bin_albedo_lambertian_hit(const uint32_t* w, int valid, uint32_t material_id, uint32_t material_count, uint32_t* material_index, uint32_t* ts) {
    if (!dn_albedo_has_record(valid, material_id, material_count)) return false;
    const uint32_t mi = PT_MATERIAL_INDEX(material_id), m = w[PT_HDR_MATERIAL_OFF] + mi * PT_MAT_WORDS;
    if (w[m + PT_MAT_KIND] != (uint32_t)PT_MATERIAL_LAMBERTIAN) return false;
    *material_index = mi; *ts = w[m + PT_MAT_TEXSTACK];
    return true;
}
// A_b(p) = (sum over the K guide samples in order, from 0.0f) / (float)K
PT_HD float dn_bin_albedo_finish(float sum, uint32_t samples) { return sum / (float)samples; }

// ---- the bins divided by the per-bin albedo before the passes, and multiplied by it after the last
PT_HD float dn_bin_divisor(float a) { return pt_max(a, DN_ALBEDO_FLOOR); }
PT_HD float dn_bin_remodulate(float s, float a) { return s * dn_bin_divisor(a); }
// One pixel before the passes.  s_b' = s_b / max(A_b, DN_ALBEDO_FLOOR); the pixel is dead when `flags` (k_dn_prepare's, or k_dn_prepare_albedo's) says so,
// or when a bin is not finite before or after the division; a dead pixel keeps the bins it came with.  Returns DN_DEAD or 0.
//   `raw`: float (uint32_t b), s_b    `alb`: float (uint32_t b), A_b (1.0f where there is no per-bin albedo: x / 1.0f is exact)
//   `store`: void (uint32_t b, float value), into planes that `raw` does not read
template <class Raw, class Alb, class Store>
PT_HD uint32_t dn_bins_demodulate_pixel(uint32_t bins, uint32_t flags, Raw&& raw, Alb&& alb, Store&& store) {
    uint32_t dead = flags & (uint32_t)DN_DEAD;
    for (uint32_t b = 0; b < bins; ++b) {
        const float s = raw(b);
        const float q = s / dn_bin_divisor(alb(b));
        dead |= (pt_isfinite(s) && pt_isfinite(q)) ? 0u : (uint32_t)DN_DEAD;
        store(b, q);
    }
    if (dead)
        for (uint32_t b = 0; b < bins; ++b) store(b, raw(b));
    return dead;
}
// the colour of a pixel that is dead through its bins alone: what k_dn_prepare gives a dead pixel — its own film values and variance, not demodulated — so
// that it comes out of the finish as it went in
PT_HD DnColor dn_bins_dead_color(float x, float y, float z, uint32_t n, double s1, double s2) { return DnColor{x, y, z, dn_variance(n, s1, s2)}; }

}  // namespace ptd
#undef DN_UNROLL
#endif
