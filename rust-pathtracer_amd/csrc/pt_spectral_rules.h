// pt_spectral_rules.h — the rules of the wavelength-binned film (include/pt_spectral.h) as PT_HD functions that the engine's
// kernel (pt_spectral.hip) and the host emulation of the tests (tests/host_emulation/ptemu_spectral.cpp) both compile: one text, so the two agree
// bit for bit.  Every accumulator is reached through an accessor `acc(b) -> float&`: the kernel hands in its column of LDS, the emulation a plain array.
#ifndef PT_SPECTRAL_RULES_H
#define PT_SPECTRAL_RULES_H
#include "pt_stages.h"

namespace ptd {

// The bin of a wavelength: x = (lambda - lo) / (span / (float)bins), b = x < 0 ? 0 : min((uint32_t)x, bins - 1).  Written so that the conversion
// only ever sees a value in [0, bins): a NaN x (a NaN lambda, or 0 / 0 with span 0) goes to bin 0, +inf to the last bin.
PT_HD uint32_t spectral_bin(float lo, float span, uint32_t bins, float lambda) {
    const float x = (lambda - lo) / (span / (float)bins);
    if (!(x >= 0.0f)) return 0u;
    if (x >= (float)bins) return bins - 1u;
    return (uint32_t)x;
}

// One sample: wavelength sample u (hero_lambdas' argument), energies e[0 .. NL-1].  NL = 1: S[b] += e; NL = 4: S[b_k] += e_k / 4.0f, k in order.
template <int NL, typename Acc>
PT_HD void spectral_add_sample(const RenderParams& rp, uint32_t bins, float u, const float* e, Acc&& acc) {
    float lam[NL];
    hero_lambdas<NL>(rp, u, lam);
    if (NL == 1) {
        acc(spectral_bin(rp.wavelength_lo, rp.wavelength_span, bins, lam[0])) += e[0];
    } else {
        for (int k = 0; k < NL; ++k) acc(spectral_bin(rp.wavelength_lo, rp.wavelength_span, bins, lam[k])) += e[k] / 4.0f;
    }
}

// One pass over pixel `pixel`, item p of the pass: its rp.pass_samples samples in order, read where stage_accumulate_pixel reads them (slot = s_local *
// chunk_pixels + p, plane k at k * energy_stride, the wavelength samples in plane NL), then the division that ends a normalised range.
template <int NL, typename Acc>
PT_HD void spectral_fold_pixel(const RenderParams& rp, uint32_t bins, const float* energy, uint32_t p, uint32_t pixel, Acc&& acc) {
    for (uint32_t s_local = 0; s_local < rp.pass_samples; ++s_local) {
        const size_t slot = (size_t)s_local * rp.chunk_pixels + p;
        float e[NL];
        for (int k = 0; k < NL; ++k) e[k] = energy[(size_t)k * rp.energy_stride + slot];
        const float u = PT_STORED_WAVELENGTH ? energy[(size_t)NL * rp.energy_stride + slot] : pt_draw4(rp.seed, pixel, rp.first_sample + s_local, PT_DIM_FILM).z;
        spectral_add_sample<NL>(rp, bins, u, e, acc);
    }
    if (rp.normalize && rp.first_sample + rp.pass_samples == rp.range_end) {
        const float n = (float)rp.spp;
        for (uint32_t b = 0; b < bins; ++b) acc(b) /= n;
    }
}

// The end of an adaptive render (pt_render_adaptive_spectral): a bin's running sum S of a pixel that took n samples becomes S / (float)n — the division
// spectral_fold_pixel makes at the end of a whole range of n samples.  n = 0 (a pixel no pass touched) leaves the 0 it holds.
PT_HD float spectral_finish_value(float S, uint32_t n) { return n == 0u ? S : S / (float)n; }

}  // namespace ptd
#endif
