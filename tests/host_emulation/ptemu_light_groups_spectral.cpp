// ptemu_light_groups_spectral.cpp — TEST HARNESS: spectral light groups (include/pt_light_groups_spectral.h) on the CPU.  Linked into the
// emulation library beside ptemu.cpp and ptemu_light_groups.cpp (tests/test_light_groups_spectral.py builds it); not part of the product.
//
// ptemu_render_light_groups_spectral is ptemu_light_groups.cpp's render loop — one wavelength, the plain walk, the FULL vertex form, the engine's routing text —
// with two more folds behind every pass: the total bins by spectral_fold_pixel<1>, the spectral film's rule, and every group's bins by lg_spectral_fold_pixel
// (pt_light_groups_spectral_rules.h), the text the engine's kernel compiles.  ptemu_render_spectral is that loop with one group of everything and the group
// outputs dropped: pt_render_spectral under the conditions of a group render.  The matrix, its refusals and the argument checks are pt_scene_host.cpp's, the ones
// the engine runs; the re-lamp runs spectral_project_pixel<KC> in the launcher's grouping.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../rust-pathtracer_amd/csrc/pt_light_groups_spectral_rules.h"
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
    const LightGroupTable table{gd->instance_group, gd->environment_group, gd->group_count};
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
    uint32_t capacity = 1u << 16;   // (ptemu_render's, and its switch)
    if (const char* cap_env = getenv("PTEMU_BATCH")) capacity = (uint32_t)strtoul(cap_env, nullptr, 10);
    RenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.seed = rd.seed; rp.width = rd.width; rp.height = rd.height;
    rp.min_bounces = rd.min_bounces; rp.max_bounces = rd.max_bounces; rp.light_samples = rd.light_samples; rp.only_direct = rd.only_direct;
    rp.wavelength_lo = rd.wavelength_lo; rp.wavelength_span = rd.wavelength_hi - rd.wavelength_lo;
    rp.spp = rd.spp; rp.range_end = rd.first_sample + rd.sample_count;
    rp.normalize = 1u;   // (the whole sample range: check_light_groups_args)
    rp.phase = rd.phase_samples;
    rp.energy_stride = capacity;
    rp.camera = pth::camera_params(sc->host.cameras[rd.camera_index], (float)rd.width / (float)rd.height);
    rp.camera_record = 1u;
    typedef Layout<1> LY;
    const size_t cap64 = ((size_t)capacity + 63u) & ~(size_t)63u;
    std::vector<uint32_t> pa((size_t)LY::path_fields * cap64), pb((size_t)LY::path_fields * cap64), ph((size_t)HS_FIELDS * cap64),
        psh((size_t)LY::shadow_fields(PT_MAX_LIGHT_SAMPLES) * cap64);
    std::vector<float> energy((size_t)lg_planes(G) * capacity);
    Queue qa{pa.data(), capacity, LY::path_fields}, qb{pb.data(), capacity, LY::path_fields}, qh{ph.data(), capacity, HS_FIELDS}, qs{psh.data(), capacity, LY::shadow_fields(PT_MAX_LIGHT_SAMPLES)};
    uint64_t bounce_rays = 0, shadow_rays = 0, env_hits = 0, camera_rays = 0;
    const uint32_t bounce_limit = rd.only_direct ? 1u : rd.max_bounces;
    const bool certs = (bu(s, PT_HDR_FLAGS) & PT_FLAG_CONVEX) && bu(s, PT_HDR_CONVEX_INST) != 0u;
    for (const pth::Pass& pass : pth::plan_passes((uint32_t)pixels.size(), rd.first_sample, rd.sample_count, capacity, rd.phase_samples)) {
        rp.chunk_pixels = pass.pixel_count; rp.first_sample = pass.first_sample; rp.pass_samples = pass.sample_count;
        const uint32_t* px = pixels.data() + pass.pixel_begin;
        const uint32_t n = pass.pixel_count * pass.sample_count;
        camera_rays += n;
        for (uint32_t i = 0; i < n; ++i) {
            float u = 0.0f;
            const PathVertexT<1> pg = stage_generate<1>(rp, i, px[i % rp.chunk_pixels], &u);
            store_path_camera<1>(qa, i, pg);
            energy[i] = 0.0f; energy[(size_t)capacity + i] = u;
            for (uint32_t g = 0; g < G; ++g) energy[(size_t)lg_plane(g) * capacity + i] = 0.0f;
        }
        uint32_t live = n;
        for (uint32_t bounce = 0; bounce < bounce_limit; ++bounce) {
            Queue qin = (bounce & 1) ? qb : qa, qout = (bounce & 1) ? qa : qb;
            for (uint32_t i = 0; i < live; ++i) {
                Hit h;
                const bool marked = bounce > 0 && certs && qf(qin, PS_PREV_PDF, i) < 0.0f;
                const bool inside = bounce > 0 && certs && (qu(qin, PS_SLOT, i) & PT_PATH_INSIDE_MARK) != 0u;
                world_hit(s, f3(qf(qin, PS_OX, i), qf(qin, PS_OY, i), qf(qin, PS_OZ, i)), f3(qf(qin, PS_DX, i), qf(qin, PS_DY, i), qf(qin, PS_DZ, i)), &h, PT_INF, PT_STOP_NONE, 0xffffffffu, 0.0f,
                          marked ? bu(s, PT_HDR_CONVEX_INST) - 1u : 0xffffffffu, inside ? bu(s, PT_HDR_CONVEX_INST) - 1u : 0xffffffffu);
                store_hit(qh, i, h);
            }
            uint32_t next = 0, items = 0;
            for (uint32_t i = 0; i < live; ++i) {
                PathVertexT<1> pv = load_path<1>(qin, i, bounce == 0u);
                if (bounce > 0) pv.slot &= ~PT_PATH_INSIDE_MARK;
                const Hit hit = load_hit(qh, i);
                const bool wants = shade_wants_item(s, rp, hit);
                const uint32_t ipos = items;
                const ShadeOutT<1> out = stage_shade<1, true, true>(s, rp, bounce, pv, hit, px[pv.slot % rp.chunk_pixels],
                                                                    [&](uint32_t l, const ShadowRayT<1>& ray) { store_shadow_ray<1>(qs, ipos, l, ray); });
                if (wants) {
                    items++;
                    qsu(qs, LY::sh_slot, ipos, pv.slot); qsu(qs, LY::sh_flags, ipos, out.env_mask); qsf(qs, LY::sh_lambda, ipos, pv.lambda);
                    if (!out.has_item) clear_shadow_item<1>(qs, ipos, rp.light_samples);
                }
                if (out.add_energy) {
                    energy[pv.slot] += out.energy_add[0];
                    lg_add_vertex(s, table, hit, out.energy_add[0], energy.data(), capacity, pv.slot);
                }
                if (out.survives) store_path<1>(qout, next++, out.next);
                bounce_rays += out.vertex_pushed; env_hits += out.env_hit; shadow_rays += out.shadow_count;
            }
            for (uint32_t i = 0; i < items; ++i) lg_shadow_item<PT_TRAV_ANY>(s, table, rp.light_samples, qs, i, energy.data(), capacity);
            live = next;
        }
        if (sample_energy)   // (ptemu_light_groups_spectral_samples: what the folds below read)
            for (uint32_t p = 0; p < rp.chunk_pixels; ++p)
                for (uint32_t sl = 0; sl < rp.pass_samples; ++sl) {
                    const size_t slot = (size_t)sl * rp.chunk_pixels + p, at = (size_t)(rp.first_sample + sl) * film_pixels + px[p];
                    sample_u[at] = energy[(size_t)capacity + slot];
                    for (uint32_t g = 0; g < G; ++g) sample_energy[(size_t)g * rd.spp * film_pixels + at] = energy[(size_t)lg_plane(g) * capacity + slot];
                }
        for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
            stage_accumulate_pixel<1>(rp, energy.data(), p, px[p], film + 4 * (size_t)px[p]);
            float* total = spectral + px[p];
            spectral_fold_pixel<1>(rp, bins, energy.data(), p, px[p], [&](uint32_t b) -> float& { return total[(size_t)b * film_pixels]; });
            for (uint32_t g = 0; g < G; ++g) {
                lg_accumulate_pixel(rp, energy.data(), g, p, px[p], group_films + 4 * ((size_t)g * film_pixels + px[p]));
                float* own = group_spectral + (size_t)g * bins * film_pixels + px[p];
                lg_spectral_fold_pixel(rp, bins, energy.data(), g, p, [&](uint32_t b) -> float& { return own[(size_t)b * film_pixels]; });
            }
        }
    }
    if (profile) {
        std::memset(profile, 0, sizeof(*profile));
        profile->camera_rays = camera_rays; profile->bounce_rays = bounce_rays + camera_rays; profile->shadow_rays = shadow_rays; profile->env_hits = env_hits;
    }
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
