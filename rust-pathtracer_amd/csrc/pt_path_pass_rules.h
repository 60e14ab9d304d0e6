// pt_path_pass_rules.h — the rules of path passes (include/pt_light_groups.h) as PT_HD functions that the kernels (pt_kern_routed.hip
// through PassRouter, below) and the host emulation of the tests (tests/host_emulation/ptemu_path_passes.cpp) both compile: one text, so they agree
// bit for bit.  All f32, no contraction, in the order written.
//
// A pass render is a group render whose group is a function of the path's own history: planes 2 + c of a pass's energy buffer (pt_light_group_rules.h) hold
// the eight classes in the order of PT_PATH_PASS_*, and everything behind the render — k_accumulate_groups, the resident group films, the mix, the joint
// filter — is the group render's.  Every addition goes to the total plane as it always did and to the plane of exactly ONE class.
//
// The state in front of a vertex is (d, k): d in {0, 1, 2} the scattering events so far, saturating; k the kind of the first one (undefined while d = 0).
// Every surface vertex the walk continues from is an event, light-tagged vertices included (lights scatter here).  A vertex addition goes to emission
// (a hit) or background (a miss) at d = 0, to k-direct at d = 1, to k-indirect at d = 2.  A light-sample ray made at a vertex with (d, k) in front of it goes
// to e(ray.d)-direct at d = 0, to k-indirect otherwise.  An item's rays therefore fall into at most two classes: class_a (the reflection side, diffuse, or
// the indirect class) and class_b (transmission direct: only at a d = 0 GGX or Passthrough vertex).
//
// One uint32 per slot, in the plane behind the class planes, carries both what the light-sample kernel of this bounce and what the vertex kernel of the next
// bounce read: bits 0..2 class_a, bits 3..5 class_b, bit 8 + l: ray l belongs to class_b (the item word), bits 16..17 d and bits 18..19 k behind this vertex
// (the state).  One path and at most one item exist per slot and bounce, a pass's stream runs shade(b), light-sample(b), extend, shade(b + 1) in order and the
// two overlap lanes own separate buffers, so the word is never read before its writer.  Bounce 0 reads none: the plane needs no clear.
#ifndef PT_PATH_PASS_RULES_H
#define PT_PATH_PASS_RULES_H
#include "pt_light_group_rules.h"

namespace ptd {

constexpr uint32_t PP_CLASSES = 8;   // PT_PATH_PASSES of the header; the indices are PT_PATH_PASS_*
constexpr uint32_t PP_EMISSION = 0, PP_BACKGROUND = 1, PP_DIFFUSE_DIRECT = 2, PP_TRANSMISSION_DIRECT = 6;
constexpr uint32_t PP_DIFFUSE = 0, PP_REFLECTION = 1, PP_TRANSMISSION = 2;   // the kind of a scattering event

PT_HD uint32_t pp_state_plane() { return lg_planes(PP_CLASSES); }       // behind the class planes
PT_HD uint32_t pp_planes() { return lg_planes(PP_CLASSES) + 1u; }       // planes of a pass render's energy buffer
// the words of a pass's state plane (one per slot) in its energy buffer
PT_HD uint32_t* pp_state_words(float* energy, uint32_t energy_stride) { return reinterpret_cast<uint32_t*>(energy + (size_t)pp_state_plane() * energy_stride); }

PT_HD uint32_t pp_direct(uint32_t kind) { return PP_DIFFUSE_DIRECT + 2u * kind; }
PT_HD uint32_t pp_indirect(uint32_t kind) { return PP_DIFFUSE_DIRECT + 2u * kind + 1u; }

PT_HD bool pp_side(F3 n, F3 v) { return ((n.x * v.x + n.y * v.y) + n.z * v.z) > 0.0f; }
// whether every event at a vertex of this material kind is diffuse (the record's kind: Lambertian, DiffuseLight, SharpLight); GGX and Passthrough split by side
PT_HD bool pp_kind_is_diffuse(uint32_t material_kind) {
    return material_kind == (uint32_t)PT_MATERIAL_LAMBERTIAN || material_kind == (uint32_t)PT_MATERIAL_DIFFUSE_LIGHT || material_kind == (uint32_t)PT_MATERIAL_SHARP_LIGHT;
}
// e(dir): the kind of the outgoing direction `dir` at a hit with normal n (hit.n as the vertex kernel holds it) and incoming direction in_d (pv.d)
PT_HD uint32_t pp_event_kind(bool diffuse, F3 n, F3 in_d, F3 dir) {
    if (diffuse) return PP_DIFFUSE;
    return pp_side(n, in_d) == pp_side(n, dir) ? PP_TRANSMISSION : PP_REFLECTION;
}

PT_HD uint32_t pp_state_d(uint32_t word) { return (word >> 16) & 3u; }
PT_HD uint32_t pp_state_k(uint32_t word) { return (word >> 18) & 3u; }
// the state behind a vertex with (d, k) in front of it whose continuation is of kind e: d' = min(d + 1, 2), k' = d == 0 ? e : k
PT_HD uint32_t pp_next_state(uint32_t d, uint32_t k, uint32_t e) {
    const uint32_t d1 = d + 1u < 2u ? d + 1u : 2u, k1 = d == 0u ? e : k;
    return d1 << 16 | k1 << 18;
}

// the class of a vertex addition (out.add_energy) at a vertex with (d, k) in front of it
PT_HD uint32_t pp_vertex_class(uint32_t d, uint32_t k, bool hit) {
    if (d == 0u) return hit ? PP_EMISSION : PP_BACKGROUND;
    return d == 1u ? pp_direct(k) : pp_indirect(k);
}
// A vertex' energy addition (`energy[slot] += add`, which the caller has made): the same addition to the plane of its class.
PT_HD void pp_add_vertex(uint32_t d, uint32_t k, bool hit, float add, float* energy, uint32_t energy_stride, uint32_t slot) {
    energy[(size_t)lg_plane(pp_vertex_class(d, k, hit)) * energy_stride + slot] += add;
}

// The item word of a vertex with (d, k) in front of it, before any ray: class_a and class_b.
PT_HD uint32_t pp_item_classes(uint32_t d, uint32_t k, bool diffuse) {
    const uint32_t a = d != 0u ? pp_indirect(k) : diffuse ? pp_direct(PP_DIFFUSE) : pp_direct(PP_REFLECTION);
    const uint32_t b = (d == 0u && !diffuse) ? PP_TRANSMISSION_DIRECT : a;
    return a | b << 3;
}
PT_HD uint32_t pp_item_class_a(uint32_t word) { return word & 7u; }
PT_HD uint32_t pp_item_class_b(uint32_t word) { return (word >> 3) & 7u; }
// ray l of the item, of direction ray_d: its bit of the item word (set: the ray belongs to class_b) — the ray sink of the vertex kernel
PT_HD uint32_t pp_item_ray_bit(uint32_t d, bool diffuse, F3 n, F3 in_d, uint32_t l, F3 ray_d) {
    return (d == 0u && pp_event_kind(diffuse, n, in_d, ray_d) == PP_TRANSMISSION) ? 0x100u << l : 0u;
}

// ray l's contribution folded into the sum of its class: the other sum is left as it is (a select, as lg_item_fold)
PT_HD void pp_item_fold(uint32_t word, uint32_t l, float contribution, float* sum_a, float* sum_b) {
    const bool in_b = ((word >> (8u + l)) & 1u) != 0u;
    *sum_a = in_b ? *sum_a : *sum_a + contribution;
    *sum_b = in_b ? *sum_b + contribution : *sum_b;
}
// the item's two sums, each / light_samples, added to the planes of its classes: class_b's only where it is a class of its own
PT_HD void pp_item_add(uint32_t word, float sum_a, float sum_b, uint32_t light_samples, float* energy, uint32_t energy_stride, uint32_t slot) {
    const uint32_t a = pp_item_class_a(word), b = pp_item_class_b(word);
    energy[(size_t)lg_plane(a) * energy_stride + slot] += sum_a / (float)light_samples;
    if (b != a) energy[(size_t)lg_plane(b) * energy_stride + slot] += sum_b / (float)light_samples;
}


// Path passes: the plane of the class of the path's own history (the rules above).  `state`: the pass's state plane, one word per slot (pp_state_words).
struct PassRouter {
    uint32_t* state;
    typedef uint32_t* __restrict__ Arg;   // (no other pointer of the kernels reaches the state plane)
    PT_ROUTER_FN Arg arg() const { return state; }
    struct Vertex { uint32_t d, k; bool diffuse; uint32_t word; };   // the state in front of the vertex, the kind of its material, the item word the rays fill
    struct Item { uint32_t word; float sum_a, sum_b; };
    PT_ROUTER_FN Vertex vertex(const SceneView& s, uint32_t bounce, uint32_t slot, const Hit& hit) const {
        const uint32_t before = bounce == 0u ? 0u : state[slot];   // (the camera vertex: d = 0, nothing read)
        Vertex v;
        v.d = pp_state_d(before); v.k = pp_state_k(before);
        v.diffuse = hit.valid ? pp_kind_is_diffuse(bu(s, material_record(s, hit.material) + PT_MAT_KIND)) : true;
        v.word = pp_item_classes(v.d, v.k, v.diffuse);
        return v;
    }
    PT_ROUTER_FN void ray(Vertex& v, const Hit& hit, F3 in_d, uint32_t l, F3 ray_d) const { v.word |= pp_item_ray_bit(v.d, v.diffuse, hit.n, in_d, l, ray_d); }
    PT_ROUTER_FN void add_vertex(const SceneView&, const Vertex& v, const Hit& hit, float add, float* energy, uint32_t energy_stride, uint32_t slot) const {
        pp_add_vertex(v.d, v.k, hit.valid, add, energy, energy_stride, slot);
    }
    PT_ROUTER_FN void leave(const Vertex& v, const Hit& hit, F3 in_d, bool survives, F3 next_d, uint32_t slot) const {
        if (hit.valid) state[slot] = v.word | (survives ? pp_next_state(v.d, v.k, pp_event_kind(v.diffuse, hit.n, in_d, next_d)) : 0u);
    }
    PT_ROUTER_FN Item item(uint32_t slot) const { return Item{state[slot], 0.0f, 0.0f}; }
    PT_ROUTER_FN void fold(const SceneView&, Item& it, uint32_t l, bool, uint32_t, float c) const { pp_item_fold(it.word, l, c, &it.sum_a, &it.sum_b); }
    PT_ROUTER_FN void add(const Item& it, uint32_t light_samples, float* energy, uint32_t energy_stride, uint32_t slot) const {
        pp_item_add(it.word, it.sum_a, it.sum_b, light_samples, energy, energy_stride, slot);
    }
};

// One light-sample item of a pass render by its earlier name and arguments (the item only reads the state plane, hence the cast): the previous revision's
// emulation sources compile against this header
template <int TRAV = PT_TRAV_ANY>
PT_HD void pp_shadow_item(const SceneView& s, uint32_t light_samples, const Queue& shadow, uint32_t item, float* energy, uint32_t energy_stride, const uint32_t* state) {
    routed_shadow_item<TRAV>(s, PassRouter{const_cast<uint32_t*>(state)}, light_samples, shadow, item, energy, energy_stride);
}

}  // namespace ptd
#endif
