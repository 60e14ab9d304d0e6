// ptemu_routed_pass.h — TEST HARNESS: the passes of a routed render (csrc/pt_routed_rules.h: light groups, path passes) on the CPU, for the emulations that
// include it (ptemu_light_groups.cpp, ptemu_adaptive_light_groups.cpp, ptemu_light_groups_spectral.cpp, ptemu_path_passes.cpp); not part of the product.
//
// routed_passes is ptemu.cpp's render loop for one wavelength and the plain walk — the vertex form the engine's routed render takes, FULL — with the engine's
// own lane bodies: the vertex step is routed_vertex, the light-sample step routed_shadow_item, the texts pt_kern_routed.hip compiles.  The total plane receives
// every addition as ptemu_render's does, the router's planes their own.  ptemu.cpp's loop is not this one: it is the independent reading the tests compare with.
#ifndef PTEMU_ROUTED_PASS_H
#define PTEMU_ROUTED_PASS_H
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../rust-pathtracer_amd/csrc/pt_path_pass_rules.h"

namespace ptemu_routed {

using namespace ptd;

// What a routed render keeps from pass to pass: the queues, the energy buffer of lg_planes(planes) planes of `capacity` slots, and the four counters.
struct Buffers {
    typedef Layout<1> LY;
    uint32_t capacity, planes;
    std::vector<uint32_t> pa, pb, ph, psh;
    std::vector<float> energy;
    Queue qa, qb, qh, qs;
    uint64_t bounce_rays = 0, shadow_rays = 0, env_hits = 0, camera_rays = 0;
    explicit Buffers(uint32_t planes_) : capacity(1u << 16), planes(planes_) {   // (ptemu_render's capacity, and its switch)
        if (const char* cap_env = getenv("PTEMU_BATCH")) capacity = (uint32_t)strtoul(cap_env, nullptr, 10);
        const size_t cap64 = ((size_t)capacity + 63u) & ~(size_t)63u;
        pa.resize((size_t)LY::path_fields * cap64); pb.resize((size_t)LY::path_fields * cap64); ph.resize((size_t)HS_FIELDS * cap64);
        psh.resize((size_t)LY::shadow_fields(PT_MAX_LIGHT_SAMPLES) * cap64);
        energy.resize((size_t)lg_planes(planes) * capacity);
        qa = Queue{pa.data(), capacity, LY::path_fields}; qb = Queue{pb.data(), capacity, LY::path_fields}; qh = Queue{ph.data(), capacity, HS_FIELDS};
        qs = Queue{psh.data(), capacity, LY::shadow_fields(PT_MAX_LIGHT_SAMPLES)};
    }
    void profile(pt_profile* p) const {
        std::memset(p, 0, sizeof(*p));
        p->camera_rays = camera_rays; p->bounce_rays = bounce_rays + camera_rays; p->shadow_rays = shadow_rays; p->env_hits = env_hits;
    }
};

// The render's parameters as far as every routed render shares them; spp, range_end and normalize are the caller's.
inline RenderParams render_params(const pth::HostScene& host, const pt_render_desc& rd, uint32_t capacity) {
    RenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.seed = rd.seed; rp.width = rd.width; rp.height = rd.height;
    rp.min_bounces = rd.min_bounces; rp.max_bounces = rd.max_bounces; rp.light_samples = rd.light_samples; rp.only_direct = rd.only_direct;
    rp.wavelength_lo = rd.wavelength_lo; rp.wavelength_span = rd.wavelength_hi - rd.wavelength_lo;
    rp.phase = rd.phase_samples;
    rp.energy_stride = capacity;
    rp.camera = pth::camera_params(host.cameras[rd.camera_index], (float)rd.width / (float)rd.height);
    rp.camera_record = 1u;
    return rp;
}

// The passes of samples [first, first + count) of the n_list pixels of `list`: film and the b.planes group films (of film_pixels float4 each) receive every pass;
// `stats` (adaptive rounds, else null): S1 / S2 per pixel too, as k_accumulate_stats gathers them.  after_pass(rp, px): behind a pass's accumulate, with the
// pass's energy buffer still whole; on_item(v, hit): routed_vertex's hook, the Router::Vertex and the hit of every vertex that wants an item.
template <typename Router, typename AfterPass, typename OnItem>
void routed_passes(const SceneView& s, RenderParams& rp, const Router& router, const pt_render_desc& rd, const uint32_t* list, uint32_t n_list, uint32_t first, uint32_t count,
                   Buffers& b, float* film, float* group_films, size_t film_pixels, double* stats, AfterPass&& after_pass, OnItem&& on_item) {
    const uint32_t capacity = b.capacity, G = b.planes;
    float* const energy = b.energy.data();
    const uint32_t bounce_limit = rd.only_direct ? 1u : rd.max_bounces;
    const bool certs = (bu(s, PT_HDR_FLAGS) & PT_FLAG_CONVEX) && bu(s, PT_HDR_CONVEX_INST) != 0u;
    rp.range_end = first + count;
    for (const pth::Pass& pass : pth::plan_passes(n_list, first, count, capacity, rd.phase_samples)) {
        rp.chunk_pixels = pass.pixel_count; rp.first_sample = pass.first_sample; rp.pass_samples = pass.sample_count;
        const uint32_t* px = list + pass.pixel_begin;
        const uint32_t n = pass.pixel_count * pass.sample_count;
        b.camera_rays += n;
        for (uint32_t i = 0; i < n; ++i) {
            float u = 0.0f;
            const PathVertexT<1> pg = stage_generate<1>(rp, i, px[i % rp.chunk_pixels], &u);
            store_path_camera<1>(b.qa, i, pg);
            energy[i] = 0.0f; energy[(size_t)capacity + i] = u;
            for (uint32_t g = 0; g < G; ++g) energy[(size_t)lg_plane(g) * capacity + i] = 0.0f;
        }
        uint32_t live = n;
        for (uint32_t bounce = 0; bounce < bounce_limit; ++bounce) {
            Queue qin = (bounce & 1) ? b.qb : b.qa, qout = (bounce & 1) ? b.qa : b.qb;
            for (uint32_t i = 0; i < live; ++i) {
                Hit h;
                const bool marked = bounce > 0 && certs && qf(qin, PS_PREV_PDF, i) < 0.0f;
                const bool inside = bounce > 0 && certs && (qu(qin, PS_SLOT, i) & PT_PATH_INSIDE_MARK) != 0u;
                world_hit(s, f3(qf(qin, PS_OX, i), qf(qin, PS_OY, i), qf(qin, PS_OZ, i)), f3(qf(qin, PS_DX, i), qf(qin, PS_DY, i), qf(qin, PS_DZ, i)), &h, PT_INF, PT_STOP_NONE, 0xffffffffu, 0.0f,
                          marked ? bu(s, PT_HDR_CONVEX_INST) - 1u : 0xffffffffu, inside ? bu(s, PT_HDR_CONVEX_INST) - 1u : 0xffffffffu);
                store_hit(b.qh, i, h);
            }
            uint32_t next = 0, items = 0;
            for (uint32_t i = 0; i < live; ++i) {
                PathVertexT<1> pv = load_path<1>(qin, i, bounce == 0u);
                if (bounce > 0) pv.slot &= ~PT_PATH_INSIDE_MARK;
                const Hit hit = load_hit(b.qh, i);
                const bool wants = shade_wants_item(s, rp, hit);
                const ShadeOutT<1> out = routed_vertex(s, rp, router, bounce, pv, hit, px[pv.slot % rp.chunk_pixels], wants, b.qs, items, energy, on_item);
                if (wants) items++;
                if (out.survives) store_path<1>(qout, next++, out.next);
                b.bounce_rays += out.vertex_pushed; b.env_hits += out.env_hit; b.shadow_rays += out.shadow_count;
            }
            for (uint32_t i = 0; i < items; ++i) routed_shadow_item<PT_TRAV_ANY>(s, router, rp.light_samples, b.qs, i, energy, capacity);
            live = next;
        }
        for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
            if (stats) stage_accumulate_pixel<1, true>(rp, energy, p, px[p], film + 4 * (size_t)px[p], stats + 2 * (size_t)px[p]);
            else stage_accumulate_pixel<1>(rp, energy, p, px[p], film + 4 * (size_t)px[p]);
            for (uint32_t g = 0; g < G; ++g) lg_accumulate_pixel(rp, energy, g, p, px[p], group_films + 4 * ((size_t)g * film_pixels + px[p]));
        }
        after_pass(rp, px);
    }
}

// a hook that does nothing
struct Nothing { template <typename... A> void operator()(const A&...) const {} };

}  // namespace ptemu_routed
#endif
