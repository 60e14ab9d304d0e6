// ptemu_light_groups.cpp — TEST HARNESS: light groups (include/pt_light_groups.h) on the CPU.  Linked into the emulation library beside
// ptemu.cpp (tests/test_light_groups.py builds it); not part of the product.
//
// ptemu_render_light_groups is the routed render's pass loop (ptemu_routed_pass.h) under the engine's GroupRouter (csrc/pt_routed_rules.h,
// pt_light_group_rules.h): the total plane receives every addition as ptemu_render's does, each group's plane its own.
// ptemu_light_groups_mix runs the mix rule, and the argument checks are pt_plan.cpp's, the ones the engine runs.
#include <string>

#include "ptemu_routed_pass.h"
#include "../../include/pt_light_groups.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

static thread_local std::string g_groups_error;

extern "C" {

const char* ptemu_light_groups_last_error(void) { return g_groups_error.c_str(); }

pt_status ptemu_render_light_groups(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gd, float* film, float* group_films, pt_profile* profile) {
    const pt_status checked = pth::check_light_groups_args(sc, rdp, gd, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film, &g_groups_error);
    if (checked != PT_OK) return checked;
    pt_render_desc rd;
    if (!pth::normalize_render_desc(*rdp, (uint32_t)sc->host.cameras.size(), &rd, &g_groups_error)) return PT_ERR_INVALID_ARGUMENT;
    const GroupRouter router{LightGroupTable{gd->instance_group, gd->environment_group, gd->group_count}};
    const uint32_t G = gd->group_count;
    const size_t film_pixels = (size_t)rd.width * rd.height;
    SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    std::vector<uint32_t> pixels = pth::shard_pixels(rd.width, rd.height, rd.tile_width, rd.tile_height, rd.shard_index, rd.shard_count);
    std::vector<float> own_group_films;
    if (!group_films) { own_group_films.resize(4 * film_pixels * G); group_films = own_group_films.data(); }
    std::memset(film, 0, sizeof(float) * 4 * film_pixels);
    std::memset(group_films, 0, sizeof(float) * 4 * film_pixels * G);
    ptemu_routed::Buffers b(G);
    RenderParams rp = ptemu_routed::render_params(sc->host, rd, b.capacity);
    rp.spp = rd.spp;
    rp.normalize = 1u;   // (the whole sample range: check_light_groups_args)
    ptemu_routed::routed_passes(s, rp, router, rd, pixels.data(), (uint32_t)pixels.size(), rd.first_sample, rd.sample_count, b, film, group_films, film_pixels, nullptr,
                                ptemu_routed::Nothing{}, ptemu_routed::Nothing{});
    if (profile) b.profile(profile);
    return PT_OK;
}

pt_status ptemu_light_groups_mix(uint32_t width, uint32_t height, uint32_t group_count, const float* group_films, const float* matrices, float* out) {
    const pt_status st = pth::check_light_groups_mix_args(width, height, group_count, group_films, matrices, out, &g_groups_error);
    if (st != PT_OK) return st;
    const size_t np = (size_t)width * height;
    for (size_t p = 0; p < np; ++p)
        lg_mix_pixel(group_count, matrices, [&](uint32_t g, float* x, float* y, float* z) { const float* v = group_films + 4 * ((size_t)g * np + p); *x = v[0]; *y = v[1]; *z = v[2]; },
                     out + 4 * p);
    return PT_OK;
}

}  // extern "C"
