// ptemu_light_groups_spectral.cpp — TEST HARNESS: spectral light groups (include/pt_light_groups_spectral.h) on the CPU.  Linked into the
// emulation library beside ptemu.cpp and ptemu_light_groups.cpp (tests/test_light_groups_spectral.py builds it); not part of the product.
//
// ptemu_render_light_groups_spectral is the routed render's pass loop (ptemu_routed_pass.h) under the engine's GroupRouter — as ptemu_light_groups.cpp runs it —
// with two more folds behind every pass: the total bins by spectral_fold_pixel<1>, the spectral film's rule, and every group's bins by lg_spectral_fold_pixel
// (pt_light_groups_spectral_rules.h), the text the engine's kernel compiles.  ptemu_render_spectral is that loop with one group of everything and the group
// outputs dropped: pt_render_spectral under the conditions of a group render.  The matrix, its refusals and the argument checks are pt_scene_host.cpp's, the ones
// the engine runs; the re-lamp runs spectral_project_pixel<KC> in the launcher's grouping.
#include <string>

#include "../../rust-pathtracer_amd/csrc/pt_light_groups_spectral_rules.h"
#include "ptemu_routed_pass.h"
#include "../../include/pt_light_groups_spectral.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

static thread_local std::string g_lgs_error;

namespace {

// what one launch of k_light_groups_relamp<KC> does, lane after lane
template <int KC>
void relamp_rows(uint32_t n_pixels, uint32_t planes, const float* matrix, const float* group_spectral, float* out) {
    for (uint32_t p = 0; p < n_pixels; ++p) {
        const float* px = group_spectral + p;
        float* o = out + p;
        spectral_project_pixel<KC>(
            planes, [&](uint32_t i) { return px[(size_t)i * n_pixels]; }, [&](int k, uint32_t i) { return matrix[(uint32_t)k * planes + i]; },
            [&](int k, float v) { o[(size_t)k * n_pixels] = v; });
    }
}

// the group render with the bins; group_films, spectral and group_spectral may be null
pt_status render(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gd, uint32_t bins, float* film, float* group_films, float* spectral,
                 float* group_spectral, pt_profile* profile, float* sample_energy = nullptr, float* sample_u = nullptr) {
    pt_render_desc rd;
    if (!pth::normalize_render_desc(*rdp, (uint32_t)sc->host.cameras.size(), &rd, &g_lgs_error)) return PT_ERR_INVALID_ARGUMENT;
    const GroupRouter router{LightGroupTable{gd->instance_group, gd->environment_group, gd->group_count}};
    const uint32_t G = gd->group_count;
    const size_t film_pixels = (size_t)rd.width * rd.height;
    SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    std::vector<uint32_t> pixels = pth::shard_pixels(rd.width, rd.height, rd.tile_width, rd.tile_height, rd.shard_index, rd.shard_count);
    std::vector<float> own_group_films, own_spectral, own_group_spectral;
    if (!group_films) { own_group_films.resize(4 * film_pixels * G); group_films = own_group_films.data(); }
    if (!spectral) { own_spectral.resize(film_pixels * bins); spectral = own_spectral.data(); }
    if (!group_spectral) { own_group_spectral.resize(film_pixels * bins * G); group_spectral = own_group_spectral.data(); }
    std::memset(film, 0, sizeof(float) * 4 * film_pixels);
    std::memset(group_films, 0, sizeof(float) * 4 * film_pixels * G);
    std::memset(spectral, 0, sizeof(float) * film_pixels * bins);
    std::memset(group_spectral, 0, sizeof(float) * film_pixels * bins * G);
    ptemu_routed::Buffers b(G);
    RenderParams rp = ptemu_routed::render_params(sc->host, rd, b.capacity);
    rp.spp = rd.spp;
    rp.normalize = 1u;   // (the whole sample range: check_light_groups_args)
    const uint32_t capacity = b.capacity;
    const float* energy = b.energy.data();
    const auto folds = [&](const RenderParams& rp, const uint32_t* px) {   // behind every pass, from the pass's energy buffer
        if (sample_energy)   // (ptemu_light_groups_spectral_samples: what the folds below read)
            for (uint32_t p = 0; p < rp.chunk_pixels; ++p)
                for (uint32_t sl = 0; sl < rp.pass_samples; ++sl) {
                    const size_t slot = (size_t)sl * rp.chunk_pixels + p, at = (size_t)(rp.first_sample + sl) * film_pixels + px[p];
                    sample_u[at] = energy[(size_t)capacity + slot];
                    for (uint32_t g = 0; g < G; ++g) sample_energy[(size_t)g * rd.spp * film_pixels + at] = energy[(size_t)lg_plane(g) * capacity + slot];
                }
        for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
            float* total = spectral + px[p];
            spectral_fold_pixel<1>(rp, bins, energy, p, px[p], [&](uint32_t b) -> float& { return total[(size_t)b * film_pixels]; });
            for (uint32_t g = 0; g < G; ++g) {
                float* own = group_spectral + (size_t)g * bins * film_pixels + px[p];
                lg_spectral_fold_pixel(rp, bins, energy, g, p, [&](uint32_t b) -> float& { return own[(size_t)b * film_pixels]; });
            }
        }
    };
    ptemu_routed::routed_passes(s, rp, router, rd, pixels.data(), (uint32_t)pixels.size(), rd.first_sample, rd.sample_count, b, film, group_films, film_pixels, nullptr, folds,
                                ptemu_routed::Nothing{});
    if (profile) b.profile(profile);
    return PT_OK;
}

}  // namespace

extern "C" {

const char* ptemu_light_groups_spectral_last_error(void) { return g_lgs_error.c_str(); }

pt_status ptemu_render_light_groups_spectral(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gd, const pt_spectral_desc* sd, float* film,
                                             float* group_films, float* spectral, float* group_spectral, pt_profile* profile) {
    const pt_status checked = pth::check_light_groups_spectral_args(sc, rdp, gd, sd, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film, &g_lgs_error);
    if (checked != PT_OK) return checked;
    return render(sc, rdp, gd, sd->bins, film, group_films, spectral, group_spectral, profile);
}

// pt_render_spectral where a group render is defined (one wavelength, the plain walk, the whole film and sample range): one group of everything
pt_status ptemu_render_spectral(pt_scene* sc, const pt_render_desc* rdp, const pt_spectral_desc* sd, float* film, float* spectral, pt_profile* profile) {
    pt_status st = pth::check_spectral_args(sc, rdp, sd, film, spectral, &g_lgs_error);
    if (st != PT_OK) return st;
    const uint32_t n = sc->host.blob[PT_HDR_INSTANCE_COUNT];
    const std::vector<uint8_t> ids(n ? n : 1u, 0);
    pt_light_groups_desc gd;
    std::memset(&gd, 0, sizeof(gd));
    gd.group_count = 1; gd.instance_count = n; gd.instance_group = ids.data(); gd.environment_group = 0;
    st = pth::check_light_groups_spectral_args(sc, rdp, &gd, sd, n, film, &g_lgs_error);
    if (st != PT_OK) return st;
    return render(sc, rdp, &gd, sd->bins, film, nullptr, spectral, nullptr, profile);
}

pt_status ptemu_light_groups_relamp_matrix(const pt_render_desc* rd, const pt_spectral_desc* sd, const pt_curve* curves, uint32_t curve_count, const float* curve_data,
                                           uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, uint32_t group_count,
                                           const int32_t* old_curve, const int32_t* new_curve, const float* gain, float* matrix) {
    return pth::light_groups_relamp_matrix(rd, sd, curves, curve_count, curve_data, curve_data_floats, K, responses, filter, subsamples, group_count, old_curve, new_curve,
                                           gain, matrix, &g_lgs_error);
}

// pt_light_groups_relamp: the argument check, then the launcher's grouping (SP_CHUNK responses per pass over the planes)
pt_status ptemu_light_groups_relamp(uint32_t width, uint32_t height, uint32_t group_count, uint32_t bins, uint32_t K, const float* matrix, const float* group_spectral,
                                    float* out) {
    const pt_status st = pth::check_relamp_args(width, height, group_count, bins, K, matrix, group_spectral, out, &g_lgs_error);
    if (st != PT_OK) return st;
    const uint32_t n = width * height, planes = group_count * bins;
    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)SP_CHUNK) {
        const float* m = matrix + (size_t)k0 * planes;
        float* o = out + (size_t)k0 * n;
        switch (K - k0 < (uint32_t)SP_CHUNK ? K - k0 : (uint32_t)SP_CHUNK) {
            case 1: relamp_rows<1>(n, planes, m, group_spectral, o); break;
            case 2: relamp_rows<2>(n, planes, m, group_spectral, o); break;
            case 3: relamp_rows<3>(n, planes, m, group_spectral, o); break;
            case 4: relamp_rows<4>(n, planes, m, group_spectral, o); break;
            case 5: relamp_rows<5>(n, planes, m, group_spectral, o); break;
            case 6: relamp_rows<6>(n, planes, m, group_spectral, o); break;
            case 7: relamp_rows<7>(n, planes, m, group_spectral, o); break;
            default: relamp_rows<8>(n, planes, m, group_spectral, o); break;
        }
    }
    return PT_OK;
}

// the matrix check pt_light_groups_relamp_resident runs against its resident bins
pt_status ptemu_light_groups_relamp_check_matrix(uint32_t K, uint32_t group_count, uint32_t bins, const float* matrix) {
    return pth::check_relamp_matrix(K, group_count, bins, matrix, &g_lgs_error);
}

// The samples behind the bins, for a restatement of the fold: sample_energy[(g * spp + s) * width * height + pixel] = group g's energy of sample s of the pixel,
// sample_u[s * width * height + pixel] = its wavelength sample, both as the pass's energy buffer held them when the folds read it.
pt_status ptemu_light_groups_spectral_samples(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gd, float* sample_energy, float* sample_u) {
    if (!sample_energy || !sample_u) { g_lgs_error = "sample_energy or sample_u is null"; return PT_ERR_INVALID_ARGUMENT; }
    pt_spectral_desc sd;
    std::memset(&sd, 0, sizeof(sd));
    sd.bins = 1;
    if (!rdp) { g_lgs_error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    std::vector<float> film(4 * (size_t)rdp->width * rdp->height);
    const pt_status checked = pth::check_light_groups_spectral_args(sc, rdp, gd, &sd, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film.data(), &g_lgs_error);
    if (checked != PT_OK) return checked;
    return render(sc, rdp, gd, 1, film.data(), nullptr, nullptr, nullptr, nullptr, sample_energy, sample_u);
}

}  // extern "C"
