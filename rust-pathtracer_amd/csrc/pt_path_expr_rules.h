// pt_path_expr_rules.h — the rules of path expressions (include/pt_light_groups.h "Path expressions") as PT_HD functions that the kernels
// (pt_kern_routed.hip through ExprRouter, below) and the host emulation of the tests (tests/host_emulation/ptemu_path_exprs.cpp) both compile: one text, so they
// agree bit for bit.  All f32, no contraction, in the order written.
//
// An expression render is a group render whose planes are the K expressions of a compiled program (pt_path_expr.cpp): planes 2 + e of a pass's energy buffer
// (pt_light_group_rules.h), and everything behind the render is the group render's.  Every addition goes to the total plane as it always did and to the plane of
// EVERY expression that matches its path: the program is an automaton over the path's scattering events (pp_event_kind, light-tagged vertices scatter too) whose
// states carry, per terminal symbol — a surface emitter of light group 0..7, the environment — the 8-bit mask of the expressions that accept there.
//
// The program's table (the header has the layout): 16 bytes per state, word x the three successors, 6 bits each, in the order D, R, T; words y, z, w the nine masks,
// terminal symbol s in byte s % 4 of word 1 + s / 4.  The kernels keep all 64 entries in device memory (1 KB) and load an entry with one 16-byte load.
//
// The state q in front of a vertex: `start` at the camera ray's vertex, else what the vertex before left.  A vertex addition's terminal is the hit's light group
// (a miss: the environment) and goes to the planes of q's mask there.  A light-sample ray made at the vertex continues the path by one event, the kind of its own
// direction: a diffuse vertex' rays all take delta(q, D); a GGX or Passthrough vertex' rays take delta(q, R) or delta(q, T) by their side.  Its terminal is the
// group of the light it hit, or the environment where it hit none (an environment ray that escapes; also every ray that adds 0, GroupRouter::fold's convention).
//
// One uint32 per slot, in the plane behind the K expression planes, carries both what the light-sample kernel of this bounce and what the vertex kernel of the
// next bounce read:
//   bits 0..5    state_a = delta(q, D) at a diffuse vertex, delta(q, R) otherwise
//   bits 6..11   state_b = delta(q, T), meaningful at a GGX or Passthrough vertex
//   bits 12..19  bit l: ray l of the item is a transmission ray and takes state_b
//   bits 20..25  the state behind the vertex (of a path that survives)
// Unlike PassRouter's, the ray bit is needed at every depth.  One path and at most one item exist per slot and bounce, a pass's stream runs shade(b),
// light-sample(b), extend, shade(b + 1) in order and the two overlap lanes own separate buffers, so the word is never read before its writer.  Bounce 0 reads
// none: the plane needs no clear.  Whatever the word holds, a state read from it is below 64 and the table has 64 entries.
//
// An item: eight sums; ray l's contribution is folded by select into every sum whose bit is in its mask (as lg_item_fold selects), and plane e receives
// sums[e] / light_samples if and only if some ray of the item had bit e.  So a plane's chain of additions is the same whichever other expressions are compiled
// beside it: expression e's film does not depend on the rest of the set.
#ifndef PT_PATH_EXPR_RULES_H
#define PT_PATH_EXPR_RULES_H
#include "pt_path_pass_rules.h"

namespace ptd {

constexpr uint32_t PX_MAX_EXPRS = 8;     // PT_PATH_EXPRS_MAX of the header
constexpr uint32_t PX_MAX_STATES = 64;   // PT_PATH_EXPR_STATES_MAX
constexpr uint32_t PX_ENVIRONMENT = 8;   // PT_PATH_EXPR_ENVIRONMENT: the terminal symbol of the environment

// a state's entry of the table
#if defined(__HIPCC__)
typedef uint4 PxEntry;
#else
struct alignas(16) PxEntry { uint32_t x, y, z, w; };
#endif

PT_HD uint32_t px_state_plane(uint32_t outputs) { return lg_planes(outputs); }   // behind the expression planes
PT_HD uint32_t px_planes(uint32_t outputs) { return lg_planes(outputs) + 1u; }   // planes of an expression render's energy buffer
// the words of a pass's state plane (one per slot) in its energy buffer: pp_state_words' arrangement behind K planes
PT_HD uint32_t* px_state_words(float* energy, uint32_t energy_stride, uint32_t outputs) {
    return reinterpret_cast<uint32_t*>(energy + (size_t)px_state_plane(outputs) * energy_stride);
}

// an entry as the routers hold it: four plain words, taken by value (the loaded entry itself is not kept: its words stay registers)
struct PxState { uint32_t next, m0, m1, m2; };
PT_HD PxState px_state(const PxEntry& e) { return PxState{e.x, e.y, e.z, e.w}; }
PT_HD uint32_t px_next(PxState e, uint32_t kind) { return (e.next >> (6u * kind)) & 63u; }   // delta(q, kind), kind one of PP_DIFFUSE, PP_REFLECTION, PP_TRANSMISSION
// the mask of terminal symbol t (0..8) in a state's entry
PT_HD uint32_t px_mask(PxState e, uint32_t t) {
    const uint32_t w = t < 4u ? e.m0 : t < 8u ? e.m1 : e.m2;
    return (w >> (8u * (t & 3u))) & 0xffu;
}

PT_HD uint32_t px_word_state_a(uint32_t word) { return word & 63u; }
PT_HD uint32_t px_word_state_b(uint32_t word) { return (word >> 6) & 63u; }
PT_HD bool px_word_ray_in_b(uint32_t word, uint32_t l) { return ((word >> (12u + l)) & 1u) != 0u; }
PT_HD uint32_t px_word_behind(uint32_t word) { return (word >> 20) & 63u; }
// the item word of a vertex with q's entry in front of it, before any ray
PT_HD uint32_t px_item_states(PxState q, bool diffuse) { return px_next(q, diffuse ? PP_DIFFUSE : PP_REFLECTION) | px_next(q, PP_TRANSMISSION) << 6; }
// ray l of the item, of direction ray_d: its bit of the item word
PT_HD uint32_t px_item_ray_bit(bool diffuse, F3 n, F3 in_d, uint32_t l, F3 ray_d) {
    return pp_event_kind(diffuse, n, in_d, ray_d) == PP_TRANSMISSION ? 0x1000u << l : 0u;
}

// A vertex' energy addition (made to the total plane by the caller) repeated into every plane of `mask`, in ascending plane order.
PT_HD void px_add_vertex(uint32_t mask, float add, float* energy, uint32_t energy_stride, uint32_t slot) {
#pragma unroll
    for (uint32_t e = 0; e < PX_MAX_EXPRS; ++e)
        if ((mask >> e) & 1u) energy[(size_t)lg_plane(e) * energy_stride + slot] += add;
}
// a ray's contribution folded into every sum of its mask: the other sums are left as they are (a select, as lg_item_fold)
PT_HD void px_item_fold(float (&sums)[PX_MAX_EXPRS], uint32_t mask, float contribution) {
#pragma unroll
    for (uint32_t e = 0; e < PX_MAX_EXPRS; ++e) sums[e] = ((mask >> e) & 1u) != 0u ? sums[e] + contribution : sums[e];
}
// the item's sums, each / light_samples, to the planes some ray of the item had in its mask (`any`: the OR of the rays' masks)
PT_HD void px_item_add(const float (&sums)[PX_MAX_EXPRS], uint32_t any, uint32_t light_samples, float* energy, uint32_t energy_stride, uint32_t slot) {
#pragma unroll
    for (uint32_t e = 0; e < PX_MAX_EXPRS; ++e)
        if ((any >> e) & 1u) energy[(size_t)lg_plane(e) * energy_stride + slot] += sums[e] / (float)light_samples;
}

// Path expressions: the planes of the expressions that match the path so far and its terminal (the rules above).  table: the program's 64 entries; instance_group:
// one light group id below 8 per instance, or null: every instance in group 0 (both device memory in the kernels); state: the pass's state plane (px_state_words).
struct ExprRouter {
    struct Arg { const PxEntry* table; const uint8_t* instance_group; uint32_t* state; uint32_t start; };
    Arg a;
    PT_ROUTER_FN Arg arg() const { return a; }
    struct Vertex { PxState q; bool diffuse; uint32_t word; };   // the entry of the state in front of the vertex, the kind of its material, the item word the rays fill
    struct Item { uint32_t word, any; PxState entry_a, entry_b; float sums[PX_MAX_EXPRS]; };
    // the terminal symbol of a surface emitter's instance word
    PT_ROUTER_FN uint32_t surface_terminal(const SceneView& s, uint32_t instance_word) const {
        return a.instance_group ? lg_hit_group(s, LightGroupTable{a.instance_group, 0u, 0u}, true, instance_word) & 7u : 0u;
    }
    PT_ROUTER_FN Vertex vertex(const SceneView& s, uint32_t bounce, uint32_t slot, const Hit& hit) const {
        const uint32_t q = bounce == 0u ? a.start : px_word_behind(a.state[slot]);   // (the camera vertex: nothing read)
        Vertex v;
        v.q = px_state(a.table[q]);
        v.diffuse = hit.valid ? pp_kind_is_diffuse(bu(s, material_record(s, hit.material) + PT_MAT_KIND)) : true;
        v.word = px_item_states(v.q, v.diffuse);
        return v;
    }
    PT_ROUTER_FN void ray(Vertex& v, const Hit& hit, F3 in_d, uint32_t l, F3 ray_d) const { v.word |= px_item_ray_bit(v.diffuse, hit.n, in_d, l, ray_d); }
    PT_ROUTER_FN void add_vertex(const SceneView& s, const Vertex& v, const Hit& hit, float add, float* energy, uint32_t energy_stride, uint32_t slot) const {
        px_add_vertex(px_mask(v.q, hit.valid ? surface_terminal(s, hit.instance) : PX_ENVIRONMENT), add, energy, energy_stride, slot);
    }
    PT_ROUTER_FN void leave(const Vertex& v, const Hit& hit, F3 in_d, bool survives, F3 next_d, uint32_t slot) const {
        if (hit.valid) a.state[slot] = v.word | (survives ? px_next(v.q, pp_event_kind(v.diffuse, hit.n, in_d, next_d)) << 20 : 0u);
    }
    PT_ROUTER_FN Item item(uint32_t slot) const {
        Item it;
        it.word = a.state[slot]; it.any = 0u;
        it.entry_a = px_state(a.table[px_word_state_a(it.word)]); it.entry_b = px_state(a.table[px_word_state_b(it.word)]);
        lg_item_clear(it.sums);
        return it;
    }
    PT_ROUTER_FN void fold(const SceneView& s, Item& it, uint32_t l, bool lit, uint32_t lit_instance, float c) const {
        const uint32_t t = lit ? surface_terminal(s, lit_instance) : PX_ENVIRONMENT;
        const uint32_t mask_a = px_mask(it.entry_a, t), mask_b = px_mask(it.entry_b, t);   // (both read, then a select of values: the entries stay registers)
        const uint32_t mask = px_word_ray_in_b(it.word, l) ? mask_b : mask_a;
        it.any |= mask;
        px_item_fold(it.sums, mask, c);
    }
    PT_ROUTER_FN void add(const Item& it, uint32_t light_samples, float* energy, uint32_t energy_stride, uint32_t slot) const {
        px_item_add(it.sums, it.any, light_samples, energy, energy_stride, slot);
    }
};

}  // namespace ptd
#endif
