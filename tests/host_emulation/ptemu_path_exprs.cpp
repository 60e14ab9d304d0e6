// ptemu_path_exprs.cpp — TEST HARNESS: path expressions (include/pt_light_groups.h "Path expressions") on the CPU.  Linked into an
// emulation library beside ptemu.cpp and the compiler, csrc/pt_path_expr.cpp (tests/test_path_exprs.py builds it); not part of the product.
//
// ptemu_render_path_exprs is the routed render's pass loop (ptemu_routed_pass.h) under the engine's ExprRouter (csrc/pt_path_expr_rules.h), the plane of state
// words and the item word included.  The argument checks are pt_plan.cpp's, the ones the engine runs; refusals are reported through the light-group channel
// (ptemu_light_groups_last_error).  ptemu_path_expr_compile and ptemu_path_expr_match are the product's compiler under the emulation's prefix.
#include <string>

#include "ptemu_routed_pass.h"
#include "../../rust-pathtracer_amd/csrc/pt_path_expr_rules.h"
#include "../../include/pt_light_groups.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

static thread_local std::string g_exprs_error;

extern "C" {

const char* ptemu_light_groups_last_error(void) { return g_exprs_error.c_str(); }

pt_status ptemu_path_expr_compile(const char* const* exprs, uint32_t n, uint32_t environment_group, pt_path_expr_program* program, char* err, size_t err_len) {
    return pt_path_expr_compile(exprs, n, environment_group, program, err, err_len);
}
pt_status ptemu_path_expr_match(const pt_path_expr_program* program, const char* path, uint32_t* mask) { return pt_path_expr_match(program, path, mask); }

pt_status ptemu_render_path_exprs(pt_scene* sc, const pt_render_desc* rdp, const pt_path_expr_program* program, const uint8_t* instance_group, uint32_t n_instances,
                                  float* film, float* expr_films, pt_profile* profile) {
    const pt_status checked = pth::check_path_exprs_args(sc, rdp, program, instance_group, n_instances, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film, &g_exprs_error);
    if (checked != PT_OK) return checked;
    pt_render_desc rd;
    if (!pth::normalize_render_desc(*rdp, (uint32_t)sc->host.cameras.size(), &rd, &g_exprs_error)) return PT_ERR_INVALID_ARGUMENT;
    const uint32_t K = program->outputs;
    const size_t film_pixels = (size_t)rd.width * rd.height;
    SceneView s{sc->host.blob.data(), sc->host.tex.data(), sc->host.blob.data() + sc->host.blob[PT_HDR_CORE_WORDS]};
    std::vector<uint32_t> pixels = pth::shard_pixels(rd.width, rd.height, rd.tile_width, rd.tile_height, rd.shard_index, rd.shard_count);
    std::vector<float> own_films;
    if (!expr_films) { own_films.resize(4 * film_pixels * K); expr_films = own_films.data(); }
    std::memset(film, 0, sizeof(float) * 4 * film_pixels);
    std::memset(expr_films, 0, sizeof(float) * 4 * film_pixels * K);
    ptemu_routed::Buffers b(K);
    RenderParams rp = ptemu_routed::render_params(sc->host, rd, b.capacity);
    rp.spp = rd.spp;
    rp.normalize = 1u;   // (the whole sample range: check_path_exprs_args)
    // the table as the engine uploads it: the program's states, the rest of the 64 entries zero
    std::vector<PxEntry> table(PX_MAX_STATES, PxEntry{0u, 0u, 0u, 0u});
    for (uint32_t q = 0; q < program->states; ++q) table[q] = PxEntry{program->table[q][0], program->table[q][1], program->table[q][2], program->table[q][3]};
    // (the state plane: the engine keeps it behind the expression planes of the same buffer, px_state_words; never cleared — poisoned here, so that a read before a write shows)
    std::vector<uint32_t> state((size_t)b.capacity, 0xffffffffu);
    const ExprRouter router{{table.data(), instance_group, state.data(), program->start}};
    ptemu_routed::routed_passes(s, rp, router, rd, pixels.data(), (uint32_t)pixels.size(), rd.first_sample, rd.sample_count, b, film, expr_films, film_pixels, nullptr,
                                ptemu_routed::Nothing{}, ptemu_routed::Nothing{});
    if (profile) b.profile(profile);
    return PT_OK;
}

}  // extern "C"
