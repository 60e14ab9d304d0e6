// ptemu_spectral.cpp — TEST HARNESS: the rules of the wavelength-binned film (include/pt_spectral.h) on the CPU.  A library of its
// own beside pt_plan.cpp (tests/test_spectral.py builds it); not part of the product.
//
// It does not render: ptemu.cpp's render driver is static.  Its entry points run the engine's own text (pt_spectral_rules.h, pth::check_spectral_args)
// over planes the caller gives: the bin of each wavelength, one pass of k_accumulate_spectral over energy planes in the engine's layout, the argument check.
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_spectral_rules.h"
#include "../../include/pt_spectral.h"

#if !PT_STORED_WAVELENGTH
#error "ptemu_spectral_fold takes the wavelength samples from the plane behind the energies (PT_STORED_WAVELENGTH 1)"
#endif

using namespace ptd;

static thread_local std::string g_spectral_error;

namespace {

template <int NL>
void fold(const RenderParams& rp, uint32_t bins, const float* energy, const uint32_t* pixels, size_t plane_pixels, float* spectral) {
    for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
        float* px = spectral + pixels[p];
        spectral_fold_pixel<NL>(rp, bins, energy, p, pixels[p], [&](uint32_t b) -> float& { return px[(size_t)b * plane_pixels]; });
    }
}

}  // namespace

extern "C" {

const char* ptemu_spectral_last_error(void) { return g_spectral_error.c_str(); }

// out_bin[i] = the bin of lambda[i] among `bins` equal bins over [lo, hi] (span = hi - lo, as RenderParams::wavelength_span holds it)
pt_status ptemu_spectral_bins(size_t n, float lo, float hi, uint32_t bins, const float* lambda, uint32_t* out_bin) {
    if (bins == 0 || (n && (!lambda || !out_bin))) { g_spectral_error = "bad argument"; return PT_ERR_INVALID_ARGUMENT; }
    const float span = hi - lo;
    for (size_t i = 0; i < n; ++i) out_bin[i] = spectral_bin(lo, span, bins, lambda[i]);
    return PT_OK;
}

// One pass of the spectral accumulate kernel.  energy: nl + 1 planes of energy_stride floats (plane k < nl: the energies of wavelength k; plane nl: the
// wavelength samples), slot = s_local * chunk_pixels + p; pixels: the chunk_pixels film pixel ids of the pass; spectral (in / out): bins planes of
// plane_pixels floats.  The pass covers samples [first_sample, first_sample + pass_samples) of a call that ends at range_end; `normalize`: the call
// renders the whole range of spp samples, so the pass that reaches range_end divides by (float)spp.
pt_status ptemu_spectral_fold(uint32_t nl, uint32_t bins, float lo, float hi, const float* energy, uint32_t energy_stride, uint32_t chunk_pixels,
                              uint32_t first_sample, uint32_t pass_samples, uint32_t spp, uint32_t range_end, uint32_t normalize, const uint32_t* pixels,
                              uint32_t plane_pixels, float* spectral) {
    if ((nl != 1 && nl != 4) || bins == 0 || bins > PT_SPECTRAL_MAX_BINS || !energy || !pixels || !spectral) { g_spectral_error = "bad argument"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)pass_samples * chunk_pixels > energy_stride) { g_spectral_error = "the pass does not fit the energy planes"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t p = 0; p < chunk_pixels; ++p) if (pixels[p] >= plane_pixels) { g_spectral_error = "a pixel outside the film"; return PT_ERR_INVALID_ARGUMENT; }
    RenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.wavelength_lo = lo; rp.wavelength_span = hi - lo;
    rp.chunk_pixels = chunk_pixels; rp.first_sample = first_sample; rp.pass_samples = pass_samples; rp.spp = spp; rp.range_end = range_end;
    rp.normalize = normalize; rp.energy_stride = energy_stride;
    if (nl == 4) fold<4>(rp, bins, energy, pixels, plane_pixels, spectral);
    else fold<1>(rp, bins, energy, pixels, plane_pixels, spectral);
    return PT_OK;
}

// pth::check_spectral_args as pt_render_spectral runs it (the pointers are only compared with null)
pt_status ptemu_spectral_check_args(const void* scene, const pt_render_desc* rd, const pt_spectral_desc* sd, const void* film, const void* spectral) {
    return pth::check_spectral_args(scene, rd, sd, film, spectral, &g_spectral_error);
}

pt_status ptemu_spectral_bin_centres(const pt_render_desc* rd, const pt_spectral_desc* sd, float* centres_nm) {
    return pth::spectral_bin_centres(rd, sd, centres_nm, &g_spectral_error);
}

}  // extern "C"
