// ptemu_adaptive_light_groups.cpp — TEST HARNESS: pt_render_adaptive_light_groups (include/pt_light_groups_denoise.h) on the CPU.  Linked
// into an emulation library beside ptemu.cpp, ptemu_adaptive.cpp and ptemu_light_groups.cpp (tests/test_light_groups_denoise.py builds it); not part of the product.
//
// The driver is the engine's (pt_engine.hip adaptive_rounds over render_impl's pass loop): the same argument check (pth::check_adaptive_light_groups_args), the
// same round-0 list, the decision and keep rules of pt_adaptive_select.h, and per round the group render loop of ptemu_light_groups.cpp over the round's pixel
// list and sample range — the film and the group films hold running sums (rp.normalize 0, rp.spp = max_samples) and the statistics are gathered by
// stage_accumulate_pixel as k_accumulate_stats gathers them — and at the end every pixel of the film and of every group film is divided by its own count
// (k_adaptive_finish's rule, lg_adaptive_finish_pixel).
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_adaptive_select.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../rust-pathtracer_amd/csrc/pt_light_group_rules.h"
#include "../../include/pt_light_groups_denoise.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

static thread_local std::string g_adaptive_groups_error;

extern "C" {

const char* ptemu_adaptive_light_groups_last_error(void) { return g_adaptive_groups_error.c_str(); }

pt_status ptemu_render_adaptive_light_groups(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_light_groups_desc* gd, float* film,
                                             uint32_t* sample_counts, double* stats, float* group_films, pt_profile* profile) {
    pt_render_desc rd;
    pt_adaptive_desc ad;
    const pt_status checked = pth::check_adaptive_light_groups_args(sc, rdp, adp, gd, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, sc ? (uint32_t)sc->host.cameras.size() : 0u,
                                                                    film, sample_counts, &rd, &ad, &g_adaptive_groups_error);
    if (checked != PT_OK) return checked;
    const LightGroupTable table{gd->instance_group, gd->environment_group, gd->group_count};
    const uint32_t G = gd->group_count, w = rd.width, h = rd.height;
    const size_t film_pixels = (size_t)w * h;
    SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    std::vector<uint32_t> lists[2];
    lists[0] = pth::shard_pixels(w, h, rd.tile_width, rd.tile_height, 0, 0);
    lists[1].resize(lists[0].size());
    std::vector<float> own_group_films;
    if (!group_films) { own_group_films.resize(4 * film_pixels * G); group_films = own_group_films.data(); }
    std::memset(film, 0, sizeof(float) * 4 * film_pixels);
    std::memset(group_films, 0, sizeof(float) * 4 * film_pixels * G);   // (once per render, not per round)
    std::vector<double> st2(2 * film_pixels, 0.0);
    std::vector<uint8_t> unconverged(film_pixels);
    uint32_t capacity = 1u << 16;   // (ptemu_render's, and its switch)
    if (const char* cap_env = getenv("PTEMU_BATCH")) capacity = (uint32_t)strtoul(cap_env, nullptr, 10);
    RenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.seed = rd.seed; rp.width = w; rp.height = h;
    rp.min_bounces = rd.min_bounces; rp.max_bounces = rd.max_bounces; rp.light_samples = rd.light_samples; rp.only_direct = rd.only_direct;
    rp.wavelength_lo = rd.wavelength_lo; rp.wavelength_span = rd.wavelength_hi - rd.wavelength_lo;
    rp.spp = ad.max_samples;
    rp.normalize = 0u;   // (running sums until the finish)
    rp.phase = rd.phase_samples;
    rp.energy_stride = capacity;
    rp.camera = pth::camera_params(sc->host.cameras[rd.camera_index], (float)w / (float)h);
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
    // the pass loop of one round: samples [first, first + count) of the n pixels of `list` (ptemu_light_groups.cpp's loop, with the statistics)
    const auto run_passes = [&](const uint32_t* list, uint32_t n_list, uint32_t first, uint32_t count) {
        rp.range_end = first + count;
        for (const pth::Pass& pass : pth::plan_passes(n_list, first, count, capacity, rd.phase_samples)) {
            rp.chunk_pixels = pass.pixel_count; rp.first_sample = pass.first_sample; rp.pass_samples = pass.sample_count;
            const uint32_t* px = list + pass.pixel_begin;
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
                    Hit hit;
                    const bool marked = bounce > 0 && certs && qf(qin, PS_PREV_PDF, i) < 0.0f;
                    const bool inside = bounce > 0 && certs && (qu(qin, PS_SLOT, i) & PT_PATH_INSIDE_MARK) != 0u;
                    world_hit(s, f3(qf(qin, PS_OX, i), qf(qin, PS_OY, i), qf(qin, PS_OZ, i)), f3(qf(qin, PS_DX, i), qf(qin, PS_DY, i), qf(qin, PS_DZ, i)), &hit, PT_INF, PT_STOP_NONE, 0xffffffffu, 0.0f,
                              marked ? bu(s, PT_HDR_CONVEX_INST) - 1u : 0xffffffffu, inside ? bu(s, PT_HDR_CONVEX_INST) - 1u : 0xffffffffu);
                    store_hit(qh, i, hit);
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
            for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
                stage_accumulate_pixel<1, true>(rp, energy.data(), p, px[p], film + 4 * (size_t)px[p], st2.data() + 2 * (size_t)px[p]);
                for (uint32_t g = 0; g < G; ++g) lg_accumulate_pixel(rp, energy.data(), g, p, px[p], group_films + 4 * ((size_t)g * film_pixels + px[p]));
            }
        }
    };
    uint32_t n = (uint32_t)lists[0].size(), c = 0, len = rd.spp, cur = 0, rounds = 0;
    for (;;) {   // (ptemu_adaptive.cpp's rounds)
        const uint32_t* list = lists[cur].data();
        run_passes(list, n, c, len);
        c += len;
        ++rounds;
        std::memset(unconverged.data(), 0, film_pixels);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t p = list[i];
            sample_counts[p] = c;
            unconverged[p] = adaptive_unconverged(c, st2[2 * (size_t)p], st2[2 * (size_t)p + 1], ad.rel_error, ad.abs_error) ? 1u : 0u;
        }
        uint32_t kept = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (adaptive_keep(unconverged.data(), w, h, list[i], c, ad.max_samples)) lists[cur ^ 1u][kept++] = list[i];
        if (c >= ad.max_samples || kept == 0) break;
        n = kept;
        cur ^= 1u;
        len = ad.step < ad.max_samples - c ? ad.step : ad.max_samples - c;
    }
    for (size_t p = 0; p < film_pixels; ++p) {
        lg_adaptive_finish_pixel(sample_counts[p], film + 4 * p);   // (k_adaptive_finish's rule, which the group rule restates)
        for (uint32_t g = 0; g < G; ++g) lg_adaptive_finish_pixel(sample_counts[p], group_films + 4 * ((size_t)g * film_pixels + p));
    }
    if (stats) std::memcpy(stats, st2.data(), sizeof(double) * 2 * film_pixels);
    if (profile) {
        std::memset(profile, 0, sizeof(*profile));
        profile->camera_rays = camera_rays; profile->bounce_rays = bounce_rays + camera_rays; profile->shadow_rays = shadow_rays; profile->env_hits = env_hits;
        profile->kernel_launches[5] = rounds;
    }
    return PT_OK;
}

}  // extern "C"
