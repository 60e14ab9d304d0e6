// ptemu_denoise_spectral.cpp — TEST HARNESS: pt_denoise_spectral and the rules around pt_render_adaptive_spectral (include/pt_spectral.h, DESIGN.md section
// 14) on the CPU.  Linked into an emulation library beside ptemu.cpp, ptemu_adaptive.cpp and ptemu_denoise.cpp (tests/test_denoise_spectral.py builds it);
// not part of the product.
//
// Every per-pixel rule is the engine's (pt_denoise_spectral_rules.h, pt_denoise_rules.h and pt_spectral_rules.h compiled for the host) and the argument
// checks are the engine's (pt_plan.cpp).  The emulation does not render a spectral film: ptemu.cpp's render driver is static.  The adaptive spectral render
// is represented by its finish rule and its argument checker.
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_denoise_spectral_rules.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_spectral_rules.h"
#include "../../include/pt_spectral.h"

using namespace ptd;

static thread_local std::string g_dn_spectral_error;

namespace {
struct HostSpectralSource {
    const DnColor* color_; const DnGeo* geo_; const float* tent_; const uint8_t* flags_; const float* bins_; uint32_t width; size_t plane;
    uint32_t flags(int x, int y) const { return flags_[(size_t)y * width + (size_t)x]; }
    DnColor color(int x, int y) const { return color_[(size_t)y * width + (size_t)x]; }
    DnGeo geo(int x, int y) const { return geo_[(size_t)y * width + (size_t)x]; }
    float tent(int x, int y) const { return tent_[(size_t)y * width + (size_t)x]; }
    float bin(uint32_t b, int x, int y) const { return bins_[(size_t)b * plane + (size_t)y * width + (size_t)x]; }
};
}  // namespace

extern "C" {

const char* ptemu_denoise_spectral_last_error(void) { return g_dn_spectral_error.c_str(); }

pt_status ptemu_denoise_spectral(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                 const float* spectral, float* out_film, float* out_spectral, float* out_variance) {
    pt_denoise_desc d;
    const pt_status st = pth::check_denoise_spectral_args(desc, bins, film, sample_counts, stats, guides, spectral, out_film, out_spectral, &d, &g_dn_spectral_error);
    if (st != PT_OK) return st;
    const uint32_t w = d.width, h = d.height;
    const size_t np = (size_t)w * h;
    DnParams P;
    P.width = w; P.height = h; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    std::vector<DnColor> color[2];
    color[0].resize(np); color[1].resize(np);
    std::vector<float> sp[2];
    sp[0].assign(spectral, spectral + (size_t)bins * np); sp[1].resize((size_t)bins * np);
    std::vector<DnGeo> geo(np);
    std::vector<float> tent(np), gx(np), gy(np);
    std::vector<uint8_t> flags(np);
    for (size_t p = 0; p < np; ++p) {   // k_dn_prepare, then the bins' own reason to be dead
        const float v = dn_variance(sample_counts[p], stats[2 * p], stats[2 * p + 1]);
        color[0][p] = DnColor{film[4 * p], film[4 * p + 1], film[4 * p + 2], v};
        uint32_t sky;
        geo[p] = dn_unit(guides[4 * p], guides[4 * p + 1], guides[4 * p + 2], guides[4 * p + 3], &sky);
        flags[p] = (uint8_t)(dn_dead(film[4 * p], film[4 * p + 1], film[4 * p + 2], v) | sky);
        flags[p] = (uint8_t)(flags[p] | dn_spectral_dead(bins, [&](uint32_t b) { return sp[0][(size_t)b * np + p]; }));
    }
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t p = (size_t)y * w + x;
            auto z = [&](uint32_t xx, uint32_t yy) { return guides[4 * ((size_t)yy * w + xx) + 3]; };
            gx[p] = dn_gradient(z(x > 0 ? x - 1 : x, y), z(x, y), z(x + 1 < w ? x + 1 : x, y), x, w);
            gy[p] = dn_gradient(z(x, y > 0 ? y - 1 : y), z(x, y), z(x, y + 1 < h ? y + 1 : y), y, h);
        }
    int cur = 0;
    for (uint32_t i = 0; i < d.iterations; ++i) {
        const int step = 1 << i;
        const HostSpectralSource src{color[cur].data(), geo.data(), tent.data(), flags.data(), sp[cur].data(), w, np};
        for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) tent[(size_t)y * w + x] = dn_tent_pixel(src, P, (int)x, (int)y);
        float* so = sp[cur ^ 1].data();
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t p = (size_t)y * w + x;
                DnTaps taps;
                color[cur ^ 1][p] = dn_gather_pixel_taps(src, P, step, (int)x, (int)y, gx[p], gy[p], &taps);
                dn_gather_pixel_bins(src, step, (int)x, (int)y, taps, bins, [&](uint32_t b, float v) { so[(size_t)b * np + p] = v; });
            }
        cur ^= 1;
    }
    // (the inputs were copied before the first write: out_film may be film, out_spectral may be spectral)
    for (size_t p = 0; p < np; ++p) {
        const DnColor c = color[cur][p];
        out_film[4 * p] = c.x; out_film[4 * p + 1] = c.y; out_film[4 * p + 2] = c.z; out_film[4 * p + 3] = 0.0f;
        if (out_variance) out_variance[p] = c.v;
    }
    std::memcpy(out_spectral, sp[cur].data(), sizeof(float) * (size_t)bins * np);
    return PT_OK;
}

// k_adaptive_finish_spectral over host planes: spectral[b * n_pixels + p] = spectral_finish_value(spectral[b * n_pixels + p], counts[p])
pt_status ptemu_spectral_finish(uint32_t n_pixels, uint32_t bins, const uint32_t* counts, float* spectral) {
    if (!counts || !spectral || bins == 0 || bins > PT_SPECTRAL_MAX_BINS) { g_dn_spectral_error = "bad argument"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t b = 0; b < bins; ++b)
        for (uint32_t p = 0; p < n_pixels; ++p) spectral[(size_t)b * n_pixels + p] = spectral_finish_value(spectral[(size_t)b * n_pixels + p], counts[p]);
    return PT_OK;
}

// pth::check_adaptive_spectral_args as pt_render_adaptive_spectral runs it (the pointers are only compared with null; camera_count: the scene's)
pt_status ptemu_adaptive_spectral_check_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_spectral_desc* sd, uint32_t camera_count,
                                             const void* film, const void* sample_counts, const void* spectral) {
    pt_render_desc rd_out;
    pt_adaptive_desc ad_out;
    return pth::check_adaptive_spectral_args(scene, rd, ad, sd, camera_count, film, sample_counts, spectral, &rd_out, &ad_out, &g_dn_spectral_error);
}

}  // extern "C"
