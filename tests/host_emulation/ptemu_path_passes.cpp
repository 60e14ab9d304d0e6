// ptemu_path_passes.cpp — TEST HARNESS: path passes (include/pt_light_groups.h) on the CPU.  Linked into an emulation library beside
// ptemu.cpp (tests/test_path_passes.py builds it); not part of the product.
//
// ptemu_render_path_passes is the routed render's pass loop (ptemu_routed_pass.h) under the engine's PassRouter (csrc/pt_routed_rules.h, pt_path_pass_rules.h),
// the plane of state words and the item word included.  The argument checks are pt_plan.cpp's, the ones the engine runs; refusals are reported through the
// light-group channel (ptemu_light_groups_last_error).
// ptemu_path_passes_debug_items: with recording on, every item of the last render as three words — its item word, the d in front of its vertex, the kind of
// the vertex' material record.
#include <string>

#include "ptemu_routed_pass.h"
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
    ptemu_routed::Buffers b(G);
    RenderParams rp = ptemu_routed::render_params(sc->host, rd, b.capacity);
    rp.spp = rd.spp;
    rp.normalize = 1u;   // (the whole sample range: check_path_passes_args)
    // (the state plane: the engine keeps it behind the class planes of the same buffer, pp_state_words; never cleared — poisoned here, so that a read before a write shows)
    std::vector<uint32_t> state((size_t)b.capacity, 0xffffffffu);
    ptemu_routed::routed_passes(s, rp, PassRouter{state.data()}, rd, pixels.data(), (uint32_t)pixels.size(), rd.first_sample, rd.sample_count, b, film, pass_films, film_pixels,
                                nullptr, ptemu_routed::Nothing{}, [&](const PassRouter::Vertex& v, const Hit& hit) {
                                    if (!g_record) return;
                                    g_items.push_back(v.word); g_items.push_back(v.d);
                                    g_items.push_back(hit.valid ? bu(s, material_record(s, hit.material) + PT_MAT_KIND) : 0u);
                                });
    if (profile) b.profile(profile);
    return PT_OK;
}

}  // extern "C"
