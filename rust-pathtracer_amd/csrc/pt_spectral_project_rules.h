// pt_spectral_project_rules.h — the rules of developing a spectral film (pt_spectral_project / pt_spectral_response_matrix of include/pt_spectral.h, DESIGN.md
// section 14) as PT_HD functions that the kernel (pt_spectral_project.hip), the host side (pt_scene_host.cpp) and the host emulation of the tests
// (tests/host_emulation/ptemu_spectral_project.cpp) all compile: one text, so they agree bit for bit.  All f32, no contraction, in the order written.
//
// Projection: out_k(p) = fold over b = 0 .. B-1 ascending of acc = acc + M[k][b] * S_b(p), from acc = 0.0f; the multiply and the add are two operations.
// NOTHING is special-cased: a non-finite bin makes every output of its pixel non-finite, and a zero weight does not protect against a NaN or infinite bin
// (0 * NaN = NaN, 0 * inf = NaN).  Every k is a fold of its own, so the result does not depend on how a caller groups the responses.
//
// Response matrix: with lo, hi the render's wavelength bounds, w = (hi - lo) / (float)B and n subsamples, bin b is sampled at
//     lambda_{b,j} = lo + ((float)b + ((float)j + 0.5f) / (float)n) * w,   j = 0 .. n-1
// (n = 1: (0.0f + 0.5f) / 1.0f = 0.5f, the bin centre of pt_spectral_bin_centres bit for bit), and
//     M[k][b] = (fold over j ascending of m = m + r_k(lambda_{b,j}) * f(lambda_{b,j}), from m = 0.0f) / (float)n
// without a filter the term is r_k(lambda_{b,j}) alone.  Nothing is divided by the bin width: S_b is already the energy that fell into the bin.
#ifndef PT_SPECTRAL_PROJECT_RULES_H
#define PT_SPECTRAL_PROJECT_RULES_H
#include "pt_device.h"

namespace ptd {

constexpr int SP_MAX_RESPONSES = 16;     // PT_SPECTRAL_MAX_RESPONSES of the header
constexpr int SP_MAX_SUBSAMPLES = 16;
constexpr int SP_CHUNK = 8;              // the responses one pass over the planes carries (the kernel's widest form)
constexpr int32_t SP_CIE_X = -1, SP_CIE_Y = -2, SP_CIE_Z = -3;   // PT_RESPONSE_CIE_*

// KC responses of one pixel: load(b) = S_b(p), read once per bin; weight(k, b) = M[k][b]; store(k, v).  KC is a compile-time constant and every index into
// acc is one too after unrolling: the accumulators are registers.
template <int KC, typename Load, typename Weight, typename Store>
PT_HD void spectral_project_pixel(uint32_t bins, Load&& load, Weight&& weight, Store&& store) {
    float acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = 0.0f;
#pragma unroll 4   // (four plane loads in flight per lane; the order of every fold stays b ascending)
    for (uint32_t b = 0; b < bins; ++b) {
        const float s = load(b);
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[k] = acc[k] + weight(k, b) * s;
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) store(k, acc[k]);
}

PT_HD float spectral_sample_lambda(float lo, float w, uint32_t b, uint32_t j, uint32_t n) {
    return lo + ((float)b + ((float)j + 0.5f) / (float)n) * w;
}

// r(lambda) of one response: a curve record of the view (response >= 0: its word offset is curve_offsets[response]) or a component of the colour-matching fit
PT_HD float spectral_response_value(const SceneView& s, const uint32_t* curve_offsets, int32_t response, float lambda) {
    if (response >= 0) return curve_eval(s, curve_offsets[response], lambda);
    float x, y, z;
    xyz_bar(lambda * 10.0f, &x, &y, &z);
    return response == SP_CIE_X ? x : (response == SP_CIE_Y ? y : z);
}

// M[k][b] for response `response` and the filter curve `filter` (< 0: none)
PT_HD float spectral_matrix_entry(const SceneView& s, const uint32_t* curve_offsets, int32_t response, int32_t filter, float lo, float w, uint32_t b, uint32_t n) {
    float m = 0.0f;
    for (uint32_t j = 0; j < n; ++j) {
        const float lambda = spectral_sample_lambda(lo, w, b, j, n);
        const float r = spectral_response_value(s, curve_offsets, response, lambda);
        if (filter >= 0) m = m + r * curve_eval(s, curve_offsets[filter], lambda);
        else m = m + r;
    }
    return m / (float)n;
}

}  // namespace ptd
#endif
