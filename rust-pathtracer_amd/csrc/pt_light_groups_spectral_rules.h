// pt_light_groups_spectral_rules.h — the rules of spectral light groups (include/pt_light_groups_spectral.h) as PT_HD functions that the
// kernels (pt_light_groups_spectral.hip), the host side (pt_scene_host.cpp) and the host emulation of the tests
// (tests/host_emulation/ptemu_light_groups_spectral.cpp) all compile: one text, so they agree bit for bit.  All f32, no contraction, in the order written.
//
// The fold: group g's bins of a pixel are the running sum, in sample order, of plane lg_plane(g) of the pass's energy buffer, each energy added to the bin of
// its sample's wavelength (spectral_add_sample<1>: the binning rule of the spectral film), with the wavelength samples read from plane 1 where every render keeps
// them, exactly as lg_accumulate_pixel reads them; the division by (float)spp ends a normalised range.  The accumulators are reached through an accessor
// `acc(b) -> float&`, like spectral_fold_pixel's: the kernel hands in its column of LDS, the emulation the planes themselves.
//
// The re-lamp matrix: the entry of response k, group g and bin b is gain[g] * ((fold over j ascending of m = m + t_k(lambda_{b,j}) * q_g(lambda_{b,j}), from
// 0.0f) / (float)n), t_k = r_k or r_k * f behind a filter, q_g = 1.0f for a kept group and otherwise o > 0.0f ? new(lambda) / o : 0.0f with o = old(lambda).
// The re-lamp itself is spectral_project_pixel<KC> (pt_spectral_project_rules.h) as it stands, over G * bins planes.
#ifndef PT_LIGHT_GROUPS_SPECTRAL_RULES_H
#define PT_LIGHT_GROUPS_SPECTRAL_RULES_H
#include "pt_light_group_rules.h"
#include "pt_spectral_project_rules.h"
#include "pt_spectral_rules.h"

#if !PT_STORED_WAVELENGTH
#error "a light-group render keeps its wavelength samples in plane 1 of the energy buffer (PT_STORED_WAVELENGTH 1)"
#endif

namespace ptd {

constexpr int32_t LGS_KEEP = -1;                                   // PT_RELAMP_KEEP of the header
constexpr uint32_t LGS_MAX_PLANES = LG_MAX_GROUPS * 64u;           // PT_LIGHT_GROUPS_MAX * PT_SPECTRAL_MAX_BINS

// One pass over item p of the pass for group `group`: its rp.pass_samples samples in order (slot = s_local * chunk_pixels + p), then the division that ends a
// normalised range.
template <typename Acc>
PT_HD void lg_spectral_fold_pixel(const RenderParams& rp, uint32_t bins, const float* energy, uint32_t group, uint32_t p, Acc&& acc) {
    const float* plane = energy + (size_t)lg_plane(group) * rp.energy_stride;
    const float* samples = energy + rp.energy_stride;
    for (uint32_t s_local = 0; s_local < rp.pass_samples; ++s_local) {
        const size_t slot = (size_t)s_local * rp.chunk_pixels + p;
        const float e[1] = {plane[slot]};
        spectral_add_sample<1>(rp, bins, samples[slot], e, acc);
    }
    if (rp.normalize && rp.first_sample + rp.pass_samples == rp.range_end) {
        const float n = (float)rp.spp;
        for (uint32_t b = 0; b < bins; ++b) acc(b) /= n;
    }
}

// q_g(lambda): old_curve, new_curve are indices into curve_offsets, or LGS_KEEP (the caller has refused a kept `new` beside a replaced `old`)
PT_HD float lg_relamp_ratio(const SceneView& s, const uint32_t* curve_offsets, int32_t old_curve, int32_t new_curve, float lambda) {
    if (old_curve == LGS_KEEP) return 1.0f;
    const float o = curve_eval(s, curve_offsets[old_curve], lambda);
    return o > 0.0f ? curve_eval(s, curve_offsets[new_curve], lambda) / o : 0.0f;
}

// W[(k * G + g) * bins + b] without its gain: the response, the filter (< 0: none) and the ratio at the n sample wavelengths of bin b
PT_HD float lg_relamp_matrix_entry(const SceneView& s, const uint32_t* curve_offsets, int32_t response, int32_t filter, int32_t old_curve, int32_t new_curve, float lo,
                                   float w, uint32_t b, uint32_t n) {
    float m = 0.0f;
    for (uint32_t j = 0; j < n; ++j) {
        const float lambda = spectral_sample_lambda(lo, w, b, j, n);
        float t = spectral_response_value(s, curve_offsets, response, lambda);
        if (filter >= 0) t = t * curve_eval(s, curve_offsets[filter], lambda);
        m = m + t * lg_relamp_ratio(s, curve_offsets, old_curve, new_curve, lambda);
    }
    return m / (float)n;
}

}  // namespace ptd
#endif
