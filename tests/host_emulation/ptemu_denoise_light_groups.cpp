// ptemu_denoise_light_groups.cpp — TEST HARNESS: pt_denoise_light_groups (include/pt_light_groups_denoise.h) on the CPU.  Linked into an
// emulation library beside the other ptemu_denoise*.cpp files (tests/test_light_groups_denoise.py builds it); not part of the product.
//
// Every rule is the engine's (pt_denoise_light_groups_rules.h and the rules it rests on, compiled for the host) and so is the argument check (pt_plan.cpp).  The
// steps are ptk::dn_run's group form: the film's prepare, the groups' prepare, per pass the tent and the gather with its taps kept, the two finishes.
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_denoise_light_groups_rules.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../include/pt_light_groups_denoise.h"

using namespace ptd;

static thread_local std::string g_dn_groups_error;

namespace {
struct HostGroupSource {
    const DnColor* color_; const DnGeo* geo_; const float* tent_; const uint8_t* flags_; const DnQuad* groups_; uint32_t width; size_t plane;
    uint32_t flags(int x, int y) const { return flags_[(size_t)y * width + (size_t)x]; }
    DnColor color(int x, int y) const { return color_[(size_t)y * width + (size_t)x]; }
    DnGeo geo(int x, int y) const { return geo_[(size_t)y * width + (size_t)x]; }
    float tent(int x, int y) const { return tent_[(size_t)y * width + (size_t)x]; }
    DnQuad bin4(uint32_t g, int x, int y) const { return groups_[dn_quad_index(g, plane, (size_t)y * width + (size_t)x)]; }
};
DnQuad quad_of(const float* p) { DnQuad q; q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3]; return q; }
}  // namespace

extern "C" {

const char* ptemu_denoise_light_groups_last_error(void) { return g_dn_groups_error.c_str(); }

pt_status ptemu_denoise_light_groups(const pt_denoise_desc* desc, uint32_t group_count, const float* film, const uint32_t* sample_counts, const double* stats,
                                     const float* guides, const float* albedo, const float* group_films, float* out_film, float* out_variance, float* out_group_films) {
    pt_denoise_desc d;
    const pt_status st = pth::check_denoise_light_groups_args(desc, group_count, film, sample_counts, stats, guides, albedo, group_films, out_film, out_group_films, &d,
                                                              &g_dn_groups_error);
    if (st != PT_OK) return st;
    const uint32_t w = d.width, h = d.height, G = group_count;
    const size_t np = (size_t)w * h;
    DnParams P;
    P.width = w; P.height = h; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    std::vector<DnColor> color[2];
    color[0].resize(np); color[1].resize(np);
    std::vector<DnQuad> raw(G * np), buf[2];
    for (size_t i = 0; i < G * np; ++i) raw[i] = quad_of(group_films + 4 * i);
    buf[0].resize(G * np); buf[1].resize(G * np);
    std::vector<DnAlbedo> alb(np, DnAlbedo{1.0f, 1.0f, 1.0f});
    std::vector<DnGeo> geo(np);
    std::vector<float> tent(np), gx(np), gy(np);
    std::vector<uint8_t> flags(np);
    for (size_t p = 0; p < np; ++p) {   // k_dn_prepare or k_dn_prepare_albedo, then k_dn_groups_prepare
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
        const auto load = [&](uint32_t g) { return raw[dn_quad_index(g, np, p)]; };
        const auto store = [&](uint32_t g, DnQuad q) { buf[0][dn_quad_index(g, np, p)] = q; };
        const uint32_t gdead = albedo ? dn_groups_prepare_pixel<true>(G, f, alb[p], load, store) : dn_groups_prepare_pixel<false>(G, f, alb[p], load, store);
        if (gdead && !(f & DN_DEAD)) color[0][p] = dn_bins_dead_color(c.x, c.y, c.z, sample_counts[p], stats[2 * p], stats[2 * p + 1]);
        flags[p] = (uint8_t)(f | gdead);
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
        const HostGroupSource src{color[cur].data(), geo.data(), tent.data(), flags.data(), buf[cur].data(), w, np};
        for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) tent[(size_t)y * w + x] = dn_tent_pixel(src, P, (int)x, (int)y);
        DnQuad* go = buf[cur ^ 1].data();
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t p = (size_t)y * w + x;
                DnTaps taps;
                color[cur ^ 1][p] = dn_gather_pixel_taps(src, P, step, (int)x, (int)y, gx[p], gy[p], &taps);
                dn_gather_pixel_bins4(src, step, (int)x, (int)y, taps, G, [&](uint32_t g, DnQuad v) { go[dn_quad_index(g, np, p)] = v; });
            }
        cur ^= 1;
    }
    // (the inputs were copied before the first write: out_film may be film, out_group_films may be group_films)
    for (size_t p = 0; p < np; ++p) {
        const DnColor c = albedo ? dn_remodulate(color[cur][p], alb[p], flags[p]) : color[cur][p];
        out_film[4 * p] = c.x; out_film[4 * p + 1] = c.y; out_film[4 * p + 2] = c.z; out_film[4 * p + 3] = 0.0f;
        if (out_variance) out_variance[p] = c.v;
        for (uint32_t g = 0; g < G; ++g) {
            const size_t i = dn_quad_index(g, np, p);
            const DnQuad o = albedo ? dn_groups_finish_pixel<true>(flags[p], alb[p], buf[cur][i]) : dn_groups_finish_pixel<false>(flags[p], alb[p], buf[cur][i]);
            out_group_films[4 * i] = o[0]; out_group_films[4 * i + 1] = o[1]; out_group_films[4 * i + 2] = o[2]; out_group_films[4 * i + 3] = o[3];
        }
    }
    return PT_OK;
}

}  // extern "C"
