// ptemu_path_passes.cpp — TEST HARNESS: path passes (include/pt_light_groups.h) on the CPU.  Linked into an emulation library beside
// ptemu.cpp (tests/test_path_passes.py builds it); not part of the product.
//
// ptemu_render_path_passes is ptemu_light_groups.cpp's render loop with the engine's own routing text (pt_path_pass_rules.h), the plane of state words and the
// item word included: the vertex step below is k_shade_passes' per-lane body, the light-sample step is pp_shadow_item itself.  The argument checks are
// pt_plan.cpp's, the ones the engine runs; refusals are reported through the light-group channel (ptemu_light_groups_last_error).
// ptemu_path_passes_debug_items: with recording on, every item of the last render as three words — its item word, the d in front of its vertex, the kind of
// the vertex' material record.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../rust-pathtracer_amd/csrc/pt_path_pass_rules.h"
#include "../../include/pt_light_groups.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

static thread_local std::string g_passes_error;
static bool g_record = false;
static std::vector<uint32_t> g_items;

extern "C" {

const char* ptemu_light_groups_last_error(void) { return g_passes_error.c_str(); }

void ptemu_path_passes_debug_record(int on) { g_record = on != 0; g_items.clear(); }
uint32_t ptemu_path_passes_debug_items(uint32_t* out, uint32_t capacity_words) {
    const uint32_t n = (uint32_t)g_items.size();
    if (out) std::memcpy(out, g_items.data(), sizeof(uint32_t) * (n < capacity_words ? n : capacity_words));
    return n;
}

pt_status ptemu_render_path_passes(pt_scene* sc, const pt_render_desc* rdp, const pt_path_passes_desc* pd, float* film, float* pass_films, pt_profile* profile) {
    const pt_status checked = pth::check_path_passes_args(sc, rdp, pd, film, &g_passes_error);
    if (checked != PT_OK) return checked;
    pt_render_desc rd;
    if (!pth::normalize_render_desc(*rdp, (uint32_t)sc->host.cameras.size(), &rd, &g_passes_error)) return PT_ERR_INVALID_ARGUMENT;
    const uint32_t G = PP_CLASSES;
    const size_t film_pixels = (size_t)rd.width * rd.height;
    SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    std::vector<uint32_t> pixels = pth::shard_pixels(rd.width, rd.height, rd.tile_width, rd.tile_height, rd.shard_index, rd.shard_count);
    std::vector<float> own_pass_films;
    if (!pass_films) { own_pass_films.resize(4 * film_pixels * G); pass_films = own_pass_films.data(); }
    std::memset(film, 0, sizeof(float) * 4 * film_pixels);
    std::memset(pass_films, 0, sizeof(float) * 4 * film_pixels * G);
    if (g_record) g_items.clear();
    uint32_t capacity = 1u << 16;   // (ptemu_render's, and its switch)
    if (const char* cap_env = getenv("PTEMU_BATCH")) capacity = (uint32_t)strtoul(cap_env, nullptr, 10);
    RenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.seed = rd.seed; rp.width = rd.width; rp.height = rd.height;
    rp.min_bounces = rd.min_bounces; rp.max_bounces = rd.max_bounces; rp.light_samples = rd.light_samples; rp.only_direct = rd.only_direct;
    rp.wavelength_lo = rd.wavelength_lo; rp.wavelength_span = rd.wavelength_hi - rd.wavelength_lo;
    rp.spp = rd.spp; rp.range_end = rd.first_sample + rd.sample_count;
    rp.normalize = 1u;   // (the whole sample range: check_path_passes_args)
    rp.phase = rd.phase_samples;
    rp.energy_stride = capacity;
    rp.camera = pth::camera_params(sc->host.cameras[rd.camera_index], (float)rd.width / (float)rd.height);
    rp.camera_record = 1u;
    typedef Layout<1> LY;
    const size_t cap64 = ((size_t)capacity + 63u) & ~(size_t)63u;
    std::vector<uint32_t> pa((size_t)LY::path_fields * cap64), pb((size_t)LY::path_fields * cap64), ph((size_t)HS_FIELDS * cap64),
        psh((size_t)LY::shadow_fields(PT_MAX_LIGHT_SAMPLES) * cap64);
    std::vector<float> energy((size_t)lg_planes(G) * capacity);
    // (the state plane: the engine keeps it behind the class planes of the same buffer, pp_state_words; never cleared — poisoned here, so that a read before a write shows)
    std::vector<uint32_t> state((size_t)capacity, 0xffffffffu);
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
                // (k_shade_passes' lane body from here on)
                const uint32_t before = bounce == 0u ? 0u : state[pv.slot];
                const uint32_t d = pp_state_d(before), k = pp_state_k(before);
                const uint32_t material_kind = hit.valid ? bu(s, material_record(s, hit.material) + PT_MAT_KIND) : 0u;
                const bool diffuse = hit.valid ? pp_kind_is_diffuse(material_kind) : true;
                uint32_t word = pp_item_classes(d, k, diffuse);
                const ShadeOutT<1> out = stage_shade<1, true, true>(s, rp, bounce, pv, hit, px[pv.slot % rp.chunk_pixels], [&](uint32_t l, const ShadowRayT<1>& ray) {
                    store_shadow_ray<1>(qs, ipos, l, ray);
                    word |= pp_item_ray_bit(d, diffuse, hit.n, pv.d, l, ray.d);
                });
                if (wants) {
                    items++;
                    qsu(qs, LY::sh_slot, ipos, pv.slot); qsu(qs, LY::sh_flags, ipos, out.env_mask); qsf(qs, LY::sh_lambda, ipos, pv.lambda);
                    if (!out.has_item) clear_shadow_item<1>(qs, ipos, rp.light_samples);
                    if (g_record) { g_items.push_back(word); g_items.push_back(d); g_items.push_back(material_kind); }
                }
                if (out.add_energy) {
                    energy[pv.slot] += out.energy_add[0];
                    pp_add_vertex(d, k, hit.valid, out.energy_add[0], energy.data(), capacity, pv.slot);
                }
                if (hit.valid) state[pv.slot] = word | (out.survives ? pp_next_state(d, k, pp_event_kind(diffuse, hit.n, pv.d, out.next.d)) : 0u);
                if (out.survives) store_path<1>(qout, next++, out.next);
                bounce_rays += out.vertex_pushed; env_hits += out.env_hit; shadow_rays += out.shadow_count;
            }
            for (uint32_t i = 0; i < items; ++i) pp_shadow_item<PT_TRAV_ANY>(s, rp.light_samples, qs, i, energy.data(), capacity, state.data());
            live = next;
        }
        for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
            stage_accumulate_pixel<1>(rp, energy.data(), p, px[p], film + 4 * (size_t)px[p]);
            for (uint32_t g = 0; g < G; ++g) lg_accumulate_pixel(rp, energy.data(), g, p, px[p], pass_films + 4 * ((size_t)g * film_pixels + px[p]));
        }
    }
    if (profile) {
        std::memset(profile, 0, sizeof(*profile));
        profile->camera_rays = camera_rays; profile->bounce_rays = bounce_rays + camera_rays; profile->shadow_rays = shadow_rays; profile->env_hits = env_hits;
    }
    return PT_OK;
}

}  // extern "C"
