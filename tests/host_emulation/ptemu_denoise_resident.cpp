// ptemu_denoise_resident.cpp — TEST HARNESS: the entries of include/pt_resident.h ("The resident filter") on the CPU.  Linked into an
// emulation library beside ptemu.cpp, the other ptemu_denoise*.cpp files, ptemu_guides_chain.cpp and ptemu_spectral_project.cpp
// (tests/test_denoise_resident.py builds it); not part of the product.
//
// Every rule is the engine's (pt_denoise_resident_rules.h and the headers it rests on, compiled for the host) and so are the argument checks (pt_plan.cpp's
// check_resident_*, which refuse from the same description of the resident set).  A scene's resident set lives in host vectors here; the emulation's render
// entries know nothing of it, so a film becomes resident through ptemu_resident_load alone.  The filter with resident bins runs the quad route — to quads,
// passes with dn_gather_pixel_bins4, to bins — unless PT_RESIDENT_PLANAR_GATHER asks for the plane-major emulation (ptemu_denoise_spectral_albedo).
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_denoise_resident_rules.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../include/pt_resident.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

extern "C" {
pt_status ptemu_render_guides(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, float* guides);
pt_status ptemu_render_guides_albedo(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, float* guides, float* albedo);
pt_status ptemu_render_guides_chain(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, const pt_guide_chain_desc* chain, float* guides, float* albedo);
pt_status ptemu_render_guides_bin_albedo(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t bins, float* guides,
                                         float* albedo, float* bin_albedo);
pt_status ptemu_denoise_film(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides, float* out_film,
                             float* out_variance);
pt_status ptemu_denoise_film_albedo(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                    const float* albedo, float* out_film, float* out_variance);
pt_status ptemu_denoise_spectral_albedo(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                        const float* albedo, const float* spectral, const float* bin_albedo, float* out_film, float* out_spectral, float* out_variance);
pt_status ptemu_spectral_project(uint32_t width, uint32_t height, uint32_t bins, uint32_t K, const float* matrix, const float* spectral, float* out);
}

static thread_local std::string g_resident_error;

namespace {
struct Resident {
    uint32_t parts = 0, width = 0, height = 0, bins = 0;
    std::vector<float> film, spectral, guides, albedo, bin_albedo, den_film, den_var, den_bins;
    std::vector<uint32_t> counts;
    std::vector<double> stats;
    void tidy() {
        if (!(parts & (PT_RESIDENT_BINS | PT_RESIDENT_BIN_ALBEDO | PT_RESIDENT_DENOISED_BINS))) bins = 0;
        if (!parts) width = height = 0;
    }
    struct pt_resident_info info() const { struct pt_resident_info i; i.width = width; i.height = height; i.bins = bins; i.parts = parts; return i; }
};
std::map<const pt_scene*, Resident> g_resident;   // (never erased: the tests' scenes live for the session)

struct pt_resident_info now_of(const pt_scene* sc) {
    if (sc) return g_resident[sc].info();
    struct pt_resident_info none;
    std::memset(&none, 0, sizeof(none));
    return none;
}

struct HostQuadSource {
    const DnColor* color_; const DnGeo* geo_; const float* tent_; const uint8_t* flags_; const DnQuad* quads_; uint32_t width; size_t plane;
    uint32_t flags(int x, int y) const { return flags_[(size_t)y * width + (size_t)x]; }
    DnColor color(int x, int y) const { return color_[(size_t)y * width + (size_t)x]; }
    DnGeo geo(int x, int y) const { return geo_[(size_t)y * width + (size_t)x]; }
    float tent(int x, int y) const { return tent_[(size_t)y * width + (size_t)x]; }
    DnQuad bin4(uint32_t q, int x, int y) const { return quads_[dn_quad_index(q, plane, (size_t)y * width + (size_t)x)]; }
};

// The quad route over host arrays: k_dn_prepare(_albedo), k_dn_bins_to_quads, per pass k_dn_tent and k_dn_gather_spectral_quad, k_dn_finish(_albedo) and
// k_dn_quads_to_bins, each as the loop over the pixels its lanes are.  `d`: normalised.
void quad_route(const pt_denoise_desc& d, uint32_t bins, const float* film, const uint32_t* counts, const double* stats, const float* guides, const float* albedo,
                const float* spectral, const float* bin_albedo, float* out_film, float* out_variance, float* out_bins) {
    const uint32_t w = d.width, h = d.height, quads = dn_quad_count(bins);
    const size_t np = (size_t)w * h;
    DnParams P;
    P.width = w; P.height = h; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    std::vector<DnColor> color[2];
    color[0].resize(np); color[1].resize(np);
    std::vector<DnQuad> qb[2];   // exactly Q planes of np quads each: an index past the rule's range is past the allocation
    qb[0].resize((size_t)quads * np); qb[1].resize((size_t)quads * np);
    std::vector<DnAlbedo> alb(np, DnAlbedo{1.0f, 1.0f, 1.0f});
    std::vector<DnGeo> geo(np);
    std::vector<float> tent(np), gx(np), gy(np);
    std::vector<uint8_t> flags(np);
    for (size_t p = 0; p < np; ++p) {
        const float v = dn_variance(counts[p], stats[2 * p], stats[2 * p + 1]);
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
        const uint32_t bdead = dn_bins_to_quads_pixel(bins, f, [&](uint32_t b) { return spectral[(size_t)b * np + p]; },
                                                      [&](uint32_t b) { return bin_albedo ? bin_albedo[(size_t)b * np + p] : 1.0f; },
                                                      [&](uint32_t q, DnQuad v) { qb[0][dn_quad_index(q, np, p)] = v; });
        if (bdead && !(f & DN_DEAD)) color[0][p] = dn_bins_dead_color(c.x, c.y, c.z, counts[p], stats[2 * p], stats[2 * p + 1]);
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
        const HostQuadSource src{color[cur].data(), geo.data(), tent.data(), flags.data(), qb[cur].data(), w, np};
        for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) tent[(size_t)y * w + x] = dn_tent_pixel(src, P, (int)x, (int)y);
        DnQuad* qo = qb[cur ^ 1].data();
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t p = (size_t)y * w + x;
                DnTaps taps;
                color[cur ^ 1][p] = dn_gather_pixel_taps(src, P, step, (int)x, (int)y, gx[p], gy[p], &taps);
                dn_gather_pixel_bins4(src, step, (int)x, (int)y, taps, quads, [&](uint32_t q, DnQuad v) { qo[dn_quad_index(q, np, p)] = v; });
            }
        cur ^= 1;
    }
    for (size_t p = 0; p < np; ++p) {
        const DnColor c = albedo ? dn_remodulate(color[cur][p], alb[p], flags[p]) : color[cur][p];
        out_film[4 * p] = c.x; out_film[4 * p + 1] = c.y; out_film[4 * p + 2] = c.z; out_film[4 * p + 3] = 0.0f;
        out_variance[p] = c.v;
        auto quad = [&](uint32_t q) { return qb[cur][dn_quad_index(q, np, p)]; };
        auto balb = [&](uint32_t b) { return bin_albedo[(size_t)b * np + p]; };
        auto store = [&](uint32_t b, float v) { out_bins[(size_t)b * np + p] = v; };
        if (bin_albedo) dn_quads_to_bins_pixel<true>(bins, flags[p], quad, balb, store);
        else dn_quads_to_bins_pixel<false>(bins, flags[p], quad, balb, store);
    }
}
}  // namespace

extern "C" {

const char* ptemu_resident_last_error(void) { return g_resident_error.c_str(); }

pt_status ptemu_resident_info(pt_scene* sc, struct pt_resident_info* info) {
    const pt_status st = pth::check_resident_info_args(sc, info, &g_resident_error);
    if (st != PT_OK) return st;
    *info = g_resident[sc].info();
    return PT_OK;
}

// (test hook: what a render does to the set when it starts)
void ptemu_resident_end(pt_scene* sc) { g_resident[sc] = Resident(); }

pt_status ptemu_resident_guides(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t flags) {
    pt_guide_chain_desc cd;
    pt_status st = pth::check_resident_guides_args(sc, rd, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, chain, flags, now_of(sc), &cd, &g_resident_error);
    if (st != PT_OK) return st;
    Resident& r = g_resident[sc];
    const size_t np = (size_t)r.width * r.height;
    r.parts &= ~(PT_RESIDENT_GUIDES | PT_RESIDENT_ALBEDO | PT_RESIDENT_BIN_ALBEDO | PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    r.tidy();
    const bool albedo = (flags & PT_RESIDENT_ALBEDO) != 0u, bin_albedo = (flags & PT_RESIDENT_BIN_ALBEDO) != 0u;
    r.guides.assign(4 * np, 0.0f);
    if (albedo) r.albedo.assign(4 * np, 0.0f);
    if (bin_albedo) {
        r.bin_albedo.assign((size_t)r.bins * np, 0.0f);
        st = ptemu_render_guides_bin_albedo(sc, rd, guide_samples, chain, r.bins, r.guides.data(), r.albedo.data(), r.bin_albedo.data());
    } else if (cd.max_chain > 0) {
        st = ptemu_render_guides_chain(sc, rd, guide_samples, chain, r.guides.data(), albedo ? r.albedo.data() : nullptr);
    } else if (albedo) {
        st = ptemu_render_guides_albedo(sc, rd, guide_samples, r.guides.data(), r.albedo.data());
    } else {
        st = ptemu_render_guides(sc, rd, guide_samples, r.guides.data());
    }
    if (st != PT_OK) { g_resident_error = "the guide pass failed"; return st; }
    r.parts |= PT_RESIDENT_GUIDES | (albedo ? PT_RESIDENT_ALBEDO : 0u) | (bin_albedo ? PT_RESIDENT_BIN_ALBEDO : 0u);
    return PT_OK;
}

pt_status ptemu_resident_load(pt_scene* sc, uint32_t width, uint32_t height, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats,
                              const float* spectral, const float* guides, const float* albedo, const float* bin_albedo) {
    const pt_status st = pth::check_resident_load_args(sc, width, height, bins, film, sample_counts, stats, spectral, guides, albedo, bin_albedo, now_of(sc), &g_resident_error);
    if (st != PT_OK) return st;
    Resident& r = g_resident[sc];
    const size_t np = (size_t)width * height;
    r.parts &= ~(PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    if (film) { r.film.assign(film, film + 4 * np); r.counts.assign(sample_counts, sample_counts + np); r.stats.assign(stats, stats + 2 * np); r.parts |= PT_RESIDENT_FILM; }
    if (spectral) { r.spectral.assign(spectral, spectral + (size_t)bins * np); r.parts |= PT_RESIDENT_BINS; }
    if (guides) { r.guides.assign(guides, guides + 4 * np); r.parts |= PT_RESIDENT_GUIDES; }
    if (albedo) { r.albedo.assign(albedo, albedo + 4 * np); r.parts |= PT_RESIDENT_ALBEDO; }
    if (bin_albedo) { r.bin_albedo.assign(bin_albedo, bin_albedo + (size_t)bins * np); r.parts |= PT_RESIDENT_BIN_ALBEDO; }
    r.width = width; r.height = height;
    if (spectral || bin_albedo) r.bins = bins;
    r.tidy();
    return PT_OK;
}

pt_status ptemu_denoise_resident(pt_scene* sc, const pt_resident_denoise_desc* desc, float* out_film, float* out_variance, float* out_spectral) {
    pt_denoise_desc d;
    pt_status st = pth::check_resident_denoise_args(sc, desc, out_spectral, now_of(sc), &d, &g_resident_error);
    if (st != PT_OK) return st;
    Resident& r = g_resident[sc];
    const size_t np = (size_t)r.width * r.height;
    const bool has_bins = (r.parts & PT_RESIDENT_BINS) != 0u;
    const float* albedo = (r.parts & PT_RESIDENT_ALBEDO) ? r.albedo.data() : nullptr;
    const float* bin_albedo = (has_bins && (r.parts & PT_RESIDENT_BIN_ALBEDO)) ? r.bin_albedo.data() : nullptr;
    r.parts &= ~(PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    r.den_film.assign(4 * np, 0.0f); r.den_var.assign(np, 0.0f);
    if (has_bins) r.den_bins.assign((size_t)r.bins * np, 0.0f);
    if (has_bins && !(desc->flags & PT_RESIDENT_PLANAR_GATHER))
        quad_route(d, r.bins, r.film.data(), r.counts.data(), r.stats.data(), r.guides.data(), albedo, r.spectral.data(), bin_albedo, r.den_film.data(), r.den_var.data(),
                   r.den_bins.data());
    else if (has_bins)
        st = ptemu_denoise_spectral_albedo(&d, r.bins, r.film.data(), r.counts.data(), r.stats.data(), r.guides.data(), albedo, r.spectral.data(), bin_albedo,
                                           r.den_film.data(), r.den_bins.data(), r.den_var.data());
    else if (albedo)
        st = ptemu_denoise_film_albedo(&d, r.film.data(), r.counts.data(), r.stats.data(), r.guides.data(), albedo, r.den_film.data(), r.den_var.data());
    else
        st = ptemu_denoise_film(&d, r.film.data(), r.counts.data(), r.stats.data(), r.guides.data(), r.den_film.data(), r.den_var.data());
    if (st != PT_OK) { g_resident_error = "the filter's emulation refused the resident arrays"; return st; }
    if (out_film) std::memcpy(out_film, r.den_film.data(), 16 * np);
    if (out_variance) std::memcpy(out_variance, r.den_var.data(), 4 * np);
    if (out_spectral) std::memcpy(out_spectral, r.den_bins.data(), 4 * np * r.bins);
    r.parts |= PT_RESIDENT_DENOISED | (has_bins ? PT_RESIDENT_DENOISED_BINS : 0u);
    return PT_OK;
}

pt_status ptemu_spectral_project_resident_denoised(pt_scene* sc, uint32_t K, const float* matrix, float* out) {
    const pt_status st = pth::check_resident_project_args(sc, K, matrix, out, now_of(sc), &g_resident_error);
    if (st != PT_OK) return st;
    const Resident& r = g_resident[sc];
    return ptemu_spectral_project(r.width, r.height, r.bins, K, matrix, r.den_bins.data(), out);
}

// ---- the index rule alone, for the tests' numpy restatement: plane-major bins -> Q planes of quads (4 floats each, pads included) and back, no albedo
void ptemu_bins_to_quads(uint32_t n_pixels, uint32_t bins, const float* planes, float* quads) {
    for (uint32_t p = 0; p < n_pixels; ++p)
        dn_bins_to_quads_pixel(bins, 0u, [&](uint32_t b) { return planes[(size_t)b * n_pixels + p]; }, [](uint32_t) { return 1.0f; },
                               [&](uint32_t q, DnQuad v) { for (int j = 0; j < 4; ++j) quads[4 * dn_quad_index(q, n_pixels, p) + j] = v[j]; });
}
void ptemu_quads_to_bins(uint32_t n_pixels, uint32_t bins, const float* quads, float* planes) {
    for (uint32_t p = 0; p < n_pixels; ++p)
        dn_quads_to_bins_pixel<false>(bins, 0u, [&](uint32_t q) { DnQuad v; for (int j = 0; j < 4; ++j) v[j] = quads[4 * dn_quad_index(q, n_pixels, p) + j]; return v; },
                                      [](uint32_t) { return 1.0f; }, [&](uint32_t b, float v) { planes[(size_t)b * n_pixels + p] = v; });
}
uint32_t ptemu_quad_count(uint32_t bins) { return dn_quad_count(bins); }

}  // extern "C"
