// ptemu_denoise_spectral_albedo.cpp — TEST HARNESS: pt_render_guides_bin_albedo and pt_denoise_spectral_albedo (include/pt_spectral.h, DESIGN.md section 14,
// "Demodulating the bins") on the CPU.  Linked into an emulation library beside ptemu.cpp and the other ptemu_denoise*.cpp / ptemu_guides_chain.cpp files
// (tests/test_denoise_spectral_albedo.py builds it); not part of the product.
//
// Every rule is the engine's (pt_denoise_spectral_albedo_rules.h, pt_denoise_spectral_rules.h, pt_denoise_rules.h and pt_guides_chain_rules.h compiled for the
// host) and so are the argument checks (pt_plan.cpp).  Where the engine's fold reads a layer's curve values from the table k_bin_albedo_tables wrote, the
// stack source here evaluates layer_curves at the bin's centre on the spot; where the engine keeps a compacted list of the rays still on their way, a sample
// here walks its whole chain before the next one starts (ptemu_guides_chain.cpp's walk; max_chain 0 is the first hit).
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_blob.h"
#include "../../rust-pathtracer_amd/csrc/pt_device.h"
#include "../../rust-pathtracer_amd/csrc/pt_denoise_spectral_albedo_rules.h"
#include "../../rust-pathtracer_amd/csrc/pt_guides_chain_rules.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../include/pt_spectral.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

extern "C" pt_status ptemu_intersect(pt_scene* sc, size_t n, const float* o, const float* d, pt_hit* hits);
extern "C" pt_status ptemu_camera_samples(pt_scene* sc, const pt_render_desc* rd, size_t n, const uint32_t* pixel, const uint32_t* sample, float* o, float* d, float* lambda);

static thread_local std::string g_bin_albedo_error;

namespace {
struct HostSpectralSource {
    const DnColor* color_; const DnGeo* geo_; const float* tent_; const uint8_t* flags_; const float* bins_; uint32_t width; size_t plane;
    uint32_t flags(int x, int y) const { return flags_[(size_t)y * width + (size_t)x]; }
    DnColor color(int x, int y) const { return color_[(size_t)y * width + (size_t)x]; }
    DnGeo geo(int x, int y) const { return geo_[(size_t)y * width + (size_t)x]; }
    float tent(int x, int y) const { return tent_[(size_t)y * width + (size_t)x]; }
    float bin(uint32_t b, int x, int y) const { return bins_[(size_t)b * plane + (size_t)y * width + (size_t)x]; }
};
// the texture stack of a Lambertian hit: texels from the blob, the 16 basis curves and the bins' curves evaluated on the spot
struct HostStack {
    const SceneView& s; const DnAlbedoBasis& basis; uint32_t ts; float u, v, lo, bin_width;
    uint32_t layers() const { return bu(s, ts); }
    DnTexel texel(uint32_t i) const { return dn_albedo_texel(s.w, s.tex, ts + 1u + i * PT_LAYER_WORDS, u, v); }
    DnLayerCurves curves(uint32_t i, int j) const {
        const LayerCurves c = layer_curves(s, ts + 1u + i * PT_LAYER_WORDS, basis.lambda[j]);
        return DnLayerCurves{c.c0, c.c1, c.c2, c.c3};
    }
    DnLayerCurves bin_curves(uint32_t i, uint32_t b) const {
        const LayerCurves c = layer_curves(s, ts + 1u + i * PT_LAYER_WORDS, dn_bin_centre(lo, bin_width, b));
        return DnLayerCurves{c.c0, c.c1, c.c2, c.c3};
    }
};
struct XyzBar { void operator()(float angstrom, float* x, float* y, float* z) const { xyz_bar(angstrom, x, y, z); } };
}  // namespace

extern "C" {

const char* ptemu_denoise_spectral_albedo_last_error(void) { return g_bin_albedo_error.c_str(); }

pt_status ptemu_render_guides_bin_albedo(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t bins, float* guides,
                                         float* albedo, float* bin_albedo) {
    pt_guide_chain_desc cd;
    pt_status st = pth::check_guides_bin_albedo_args(sc, rd, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, chain, bins, guides, bin_albedo, &cd, &g_bin_albedo_error);
    if (st != PT_OK) return st;
    const SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    DnAlbedoBasis B;
    dn_albedo_basis(rd->wavelength_lo, rd->wavelength_hi, XyzBar(), &B);
    const float bin_width = dn_bin_width(rd->wavelength_lo, rd->wavelength_hi, bins);
    const uint32_t n = rd->width * rd->height;
    std::vector<uint32_t> pixel(n), sample(n);
    std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n), lambda(n);
    std::vector<DnGuideSum> sums(n);
    std::vector<DnAlbedo> asums(n, DnAlbedo{0.0f, 0.0f, 0.0f});
    std::vector<float> bsums((size_t)bins * n, 0.0f);
    std::memset(sums.data(), 0, sizeof(DnGuideSum) * n);
    for (uint32_t i = 0; i < n; ++i) pixel[i] = i;
    for (uint32_t k = 0; k < guide_samples; ++k) {
        for (uint32_t i = 0; i < n; ++i) sample[i] = k;
        st = ptemu_camera_samples(sc, rd, n, pixel.data(), sample.data(), o.data(), d.data(), lambda.data());
        if (st != PT_OK) { g_bin_albedo_error = "probe failed"; return st; }
        for (uint32_t i = 0; i < n; ++i) {
            float ro[3] = {o[3 * (size_t)i], o[3 * (size_t)i + 1], o[3 * (size_t)i + 2]}, rdir[3] = {d[3 * (size_t)i], d[3 * (size_t)i + 1], d[3 * (size_t)i + 2]};
            float length = 0.0f;
            for (uint32_t v = 0;; ++v) {
                pt_hit h;
                if (ptemu_intersect(sc, 1, ro, rdir, &h) != PT_OK) { g_bin_albedo_error = "probe failed"; return PT_ERR_INVALID_ARGUMENT; }
                DnChainNext nx;
                bool follows = false;
                if (h.valid) {
                    length = length + h.t;
                    follows = dn_chain_vertex(s, sc->host.material_count, h.material, f3(h.point[0], h.point[1], h.point[2]), f3(h.normal[0], h.normal[1], h.normal[2]),
                                              h.uv[0], h.uv[1], f3(rdir[0], rdir[1], rdir[2]), lambda[i], cd.alpha_max, v, cd.max_chain, &nx);
                }
                if (follows) {
                    ro[0] = nx.o.x; ro[1] = nx.o.y; ro[2] = nx.o.z; rdir[0] = nx.d.x; rdir[1] = nx.d.y; rdir[2] = nx.d.z;
                    continue;
                }
                dn_guide_add(&sums[i], h.valid, length, h.normal[0], h.normal[1], h.normal[2]);
                auto sum = [&](uint32_t b) -> float& { return bsums[(size_t)b * n + i]; };
                DnAlbedo a{1.0f, 1.0f, 1.0f};
                uint32_t mi = 0u, ts = 0u;
                if (dn_bin_albedo_lambertian_hit(s.w, h.valid, h.material, sc->host.material_count, &mi, &ts)) {
                    const HostStack stack{s, B, ts, h.uv[0], h.uv[1], rd->wavelength_lo, bin_width};
                    a = dn_albedo_lambertian(stack, B);
                    dn_bin_albedo_add(&stack, bins, sum);
                } else {
                    dn_bin_albedo_add((const HostStack*)nullptr, bins, sum);
                }
                dn_albedo_add(&asums[i], a);
                break;
            }
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const DnGeo g = dn_guide_finish(sums[i], guide_samples);
        guides[4 * (size_t)i] = g.nx; guides[4 * (size_t)i + 1] = g.ny; guides[4 * (size_t)i + 2] = g.nz; guides[4 * (size_t)i + 3] = g.z;
        if (albedo) {
            const DnAlbedo a = dn_albedo_finish(asums[i], guide_samples);
            albedo[4 * (size_t)i] = a.x; albedo[4 * (size_t)i + 1] = a.y; albedo[4 * (size_t)i + 2] = a.z; albedo[4 * (size_t)i + 3] = 0.0f;
        }
    }
    for (size_t i = 0; i < (size_t)bins * n; ++i) bin_albedo[i] = dn_bin_albedo_finish(bsums[i], guide_samples);
    return PT_OK;
}

pt_status ptemu_denoise_spectral_albedo(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                        const float* albedo, const float* spectral, const float* bin_albedo, float* out_film, float* out_spectral, float* out_variance) {
    pt_denoise_desc d;
    const pt_status st = pth::check_denoise_spectral_albedo_args(desc, bins, film, sample_counts, stats, guides, albedo, spectral, bin_albedo, out_film, out_spectral, &d,
                                                                 &g_bin_albedo_error);
    if (st != PT_OK) return st;
    const uint32_t w = d.width, h = d.height;
    const size_t np = (size_t)w * h;
    DnParams P;
    P.width = w; P.height = h; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    std::vector<DnColor> color[2];
    color[0].resize(np); color[1].resize(np);
    const std::vector<float> raw(spectral, spectral + (size_t)bins * np);
    std::vector<float> sp[2];
    sp[0].resize((size_t)bins * np); sp[1].resize((size_t)bins * np);
    std::vector<float> balb;
    if (bin_albedo) balb.assign(bin_albedo, bin_albedo + (size_t)bins * np);
    std::vector<DnAlbedo> alb(np, DnAlbedo{1.0f, 1.0f, 1.0f});
    std::vector<DnGeo> geo(np);
    std::vector<float> tent(np), gx(np), gy(np);
    std::vector<uint8_t> flags(np);
    for (size_t p = 0; p < np; ++p) {   // k_dn_prepare or k_dn_prepare_albedo, then k_dn_demodulate_bins
        const float v = dn_variance(sample_counts[p], stats[2 * p], stats[2 * p + 1]);
        const DnColor c{film[4 * p], film[4 * p + 1], film[4 * p + 2], v};
        uint32_t dead, sky;
        if (albedo) {
            alb[p] = DnAlbedo{albedo[4 * p], albedo[4 * p + 1], albedo[4 * p + 2]};
            color[0][p] = dn_demodulate(c, alb[p], &dead);
        } else {
            color[0][p] = c;
            dead = dn_dead(c.x, c.y, c.z, c.v);
        }
        geo[p] = dn_unit(guides[4 * p], guides[4 * p + 1], guides[4 * p + 2], guides[4 * p + 3], &sky);
        const uint32_t f = dead | sky;
        const uint32_t bdead = dn_bins_demodulate_pixel(bins, f, [&](uint32_t b) { return raw[(size_t)b * np + p]; },
                                                        [&](uint32_t b) { return bin_albedo ? balb[(size_t)b * np + p] : 1.0f; },
                                                        [&](uint32_t b, float q) { sp[0][(size_t)b * np + p] = q; });
        if (bdead && !(f & DN_DEAD)) color[0][p] = dn_bins_dead_color(c.x, c.y, c.z, sample_counts[p], stats[2 * p], stats[2 * p + 1]);
        flags[p] = (uint8_t)(f | bdead);
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
        const DnColor c = albedo ? dn_remodulate(color[cur][p], alb[p], flags[p]) : color[cur][p];
        out_film[4 * p] = c.x; out_film[4 * p + 1] = c.y; out_film[4 * p + 2] = c.z; out_film[4 * p + 3] = 0.0f;
        if (out_variance) out_variance[p] = c.v;
    }
    for (uint32_t b = 0; b < bins; ++b)
        for (size_t p = 0; p < np; ++p) {
            const float s = sp[cur][(size_t)b * np + p];
            out_spectral[(size_t)b * np + p] = (bin_albedo && !(flags[p] & DN_DEAD)) ? dn_bin_remodulate(s, balb[(size_t)b * np + p]) : s;
        }
    return PT_OK;
}

}  // extern "C"
