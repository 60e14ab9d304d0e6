// ptemu_denoise_albedo.cpp — TEST HARNESS: pt_albedo_basis, pt_render_guides_albedo and pt_denoise_film_albedo (include/pt_denoise.h, DESIGN.md
// section 13) on the CPU.  Linked into an emulation library beside ptemu.cpp, ptemu_adaptive.cpp and ptemu_denoise.cpp
// (tests/test_denoise_albedo.py builds it); not part of the product.
//
// Every rule is the engine's (pt_denoise_rules.h compiled for the host) and so are the argument checks (pt_plan.cpp).  Where the engine's fold reads
// a layer's curve values from the table k_albedo_tables wrote, the stack source here evaluates layer_curves at the hit, as texstack_eval does: the
// two ways to the same values are what the GPU tier compares.
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_blob.h"
#include "../../rust-pathtracer_amd/csrc/pt_device.h"
#include "../../rust-pathtracer_amd/csrc/pt_denoise_rules.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../include/pt_denoise.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

extern "C" pt_status ptemu_intersect(pt_scene* sc, size_t n, const float* o, const float* d, pt_hit* hits);
extern "C" pt_status ptemu_camera_samples(pt_scene* sc, const pt_render_desc* rd, size_t n, const uint32_t* pixel, const uint32_t* sample, float* o, float* d, float* lambda);
extern "C" pt_status ptemu_denoise_film(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                        float* out_film, float* out_variance);

static thread_local std::string g_albedo_error;

namespace {
struct HostSource {
    const DnColor* color_; const DnGeo* geo_; const float* tent_; const uint8_t* flags_; uint32_t width;
    uint32_t flags(int x, int y) const { return flags_[(size_t)y * width + (size_t)x]; }
    DnColor color(int x, int y) const { return color_[(size_t)y * width + (size_t)x]; }
    DnGeo geo(int x, int y) const { return geo_[(size_t)y * width + (size_t)x]; }
    float tent(int x, int y) const { return tent_[(size_t)y * width + (size_t)x]; }
};
// the texture stack of a Lambertian hit: texels from the blob, curve values evaluated on the spot
struct HostStack {
    const SceneView& s; const DnAlbedoBasis& basis; uint32_t ts; float u, v;
    uint32_t layers() const { return bu(s, ts); }
    DnTexel texel(uint32_t i) const { return dn_albedo_texel(s.w, s.tex, ts + 1u + i * PT_LAYER_WORDS, u, v); }
    DnLayerCurves curves(uint32_t i, int j) const {
        const LayerCurves c = layer_curves(s, ts + 1u + i * PT_LAYER_WORDS, basis.lambda[j]);
        return DnLayerCurves{c.c0, c.c1, c.c2, c.c3};
    }
};
struct XyzBar { void operator()(float angstrom, float* x, float* y, float* z) const { xyz_bar(angstrom, x, y, z); } };
}  // namespace

extern "C" {

const char* ptemu_denoise_albedo_last_error(void) { return g_albedo_error.c_str(); }

pt_status ptemu_albedo_basis(const pt_render_desc* rd, float* lambda, float* xyz) {
    pt_status st = pth::check_albedo_basis_args(rd, lambda, xyz, &g_albedo_error);
    if (st != PT_OK) return st;
    DnAlbedoBasis B;
    dn_albedo_basis(rd->wavelength_lo, rd->wavelength_hi, XyzBar(), &B);
    std::memcpy(lambda, B.lambda, sizeof(B.lambda));
    std::memcpy(xyz, B.w, sizeof(B.w));
    return PT_OK;
}

pt_status ptemu_render_guides_albedo(pt_scene* sc, const pt_render_desc* rd, uint32_t guide_samples, float* guides, float* albedo) {
    pt_status st = pth::check_guides_args(sc, rd, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, guides, &g_albedo_error);
    if (st == PT_OK && !albedo) { g_albedo_error = "null argument"; st = PT_ERR_INVALID_ARGUMENT; }
    if (st != PT_OK) return st;
    const SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    DnAlbedoBasis B;
    dn_albedo_basis(rd->wavelength_lo, rd->wavelength_hi, XyzBar(), &B);
    const uint32_t n = rd->width * rd->height;
    std::vector<uint32_t> pixel(n), sample(n);
    std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n), lambda(n);
    std::vector<pt_hit> hits(n);
    std::vector<DnGuideSum> sums(n);
    std::vector<DnAlbedo> asums(n, DnAlbedo{0.0f, 0.0f, 0.0f});
    std::memset(sums.data(), 0, sizeof(DnGuideSum) * n);
    for (uint32_t i = 0; i < n; ++i) pixel[i] = i;
    for (uint32_t k = 0; k < guide_samples; ++k) {
        for (uint32_t i = 0; i < n; ++i) sample[i] = k;
        st = ptemu_camera_samples(sc, rd, n, pixel.data(), sample.data(), o.data(), d.data(), lambda.data());
        if (st == PT_OK) st = ptemu_intersect(sc, n, o.data(), d.data(), hits.data());
        if (st != PT_OK) { g_albedo_error = "probe failed"; return st; }
        for (uint32_t i = 0; i < n; ++i) {
            const pt_hit& h = hits[i];
            dn_guide_add(&sums[i], h.valid, h.t, h.normal[0], h.normal[1], h.normal[2]);
            DnAlbedo a{1.0f, 1.0f, 1.0f};
            if (dn_albedo_has_record(h.valid, h.material, sc->host.material_count)) {
                const uint32_t m = material_record(s, h.material);
                if (bu(s, m + PT_MAT_KIND) == (uint32_t)PT_MATERIAL_LAMBERTIAN)
                    a = dn_albedo_lambertian(HostStack{s, B, bu(s, m + PT_MAT_TEXSTACK), h.uv[0], h.uv[1]}, B);
            }
            dn_albedo_add(&asums[i], a);
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const DnGeo g = dn_guide_finish(sums[i], guide_samples);
        guides[4 * (size_t)i] = g.nx; guides[4 * (size_t)i + 1] = g.ny; guides[4 * (size_t)i + 2] = g.nz; guides[4 * (size_t)i + 3] = g.z;
        const DnAlbedo a = dn_albedo_finish(asums[i], guide_samples);
        albedo[4 * (size_t)i] = a.x; albedo[4 * (size_t)i + 1] = a.y; albedo[4 * (size_t)i + 2] = a.z; albedo[4 * (size_t)i + 3] = 0.0f;
    }
    return PT_OK;
}

pt_status ptemu_denoise_film_albedo(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                    const float* albedo, float* out_film, float* out_variance) {
    if (!albedo) return ptemu_denoise_film(desc, film, sample_counts, stats, guides, out_film, out_variance);
    pt_denoise_desc d;
    pt_status st = pth::normalize_denoise_desc(desc, film, sample_counts, stats, guides, out_film, &d, &g_albedo_error);
    if (st == PT_OK) st = pth::check_denoise_inputs(d, sample_counts, guides, &g_albedo_error);
    if (st == PT_OK) st = pth::check_denoise_albedo(d, albedo, &g_albedo_error);
    if (st != PT_OK) return st;
    const uint32_t w = d.width, h = d.height;
    const size_t np = (size_t)w * h;
    DnParams P;
    P.width = w; P.height = h; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    std::vector<DnColor> color[2];
    color[0].resize(np); color[1].resize(np);
    std::vector<DnGeo> geo(np);
    std::vector<DnAlbedo> alb(np);
    std::vector<float> tent(np), gx(np), gy(np);
    std::vector<uint8_t> flags(np);
    for (size_t p = 0; p < np; ++p) {
        const float v = dn_variance(sample_counts[p], stats[2 * p], stats[2 * p + 1]);
        alb[p] = DnAlbedo{albedo[4 * p], albedo[4 * p + 1], albedo[4 * p + 2]};
        uint32_t dead, sky;
        color[0][p] = dn_demodulate(DnColor{film[4 * p], film[4 * p + 1], film[4 * p + 2], v}, alb[p], &dead);
        geo[p] = dn_unit(guides[4 * p], guides[4 * p + 1], guides[4 * p + 2], guides[4 * p + 3], &sky);
        flags[p] = (uint8_t)(dead | sky);
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
        const HostSource src{color[cur].data(), geo.data(), tent.data(), flags.data(), w};
        for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) tent[(size_t)y * w + x] = dn_tent_pixel(src, P, (int)x, (int)y);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t p = (size_t)y * w + x;
                color[cur ^ 1][p] = dn_gather_pixel(src, P, step, (int)x, (int)y, gx[p], gy[p]);
            }
        cur ^= 1;
    }
    // (the inputs are read in full before the first write: out_film may be film)
    for (size_t p = 0; p < np; ++p) {
        const DnColor c = dn_remodulate(color[cur][p], alb[p], flags[p]);
        out_film[4 * p] = c.x; out_film[4 * p + 1] = c.y; out_film[4 * p + 2] = c.z; out_film[4 * p + 3] = 0.0f;
        if (out_variance) out_variance[p] = c.v;
    }
    return PT_OK;
}

}  // extern "C"
