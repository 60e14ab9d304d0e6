// pt_light_group_rules.h — the rules of light groups (include/pt_light_groups.h) as PT_HD functions that the kernels
// (pt_kern_routed.hip through GroupRouter, below; pt_light_groups.hip) and the host emulation of the tests (tests/host_emulation/) all compile: one
// text, so they agree bit for bit.  All f32, no contraction, in the order written.
//
// Planes of a pass's energy buffer: 0 the total, 1 the stored wavelength samples (both as every render has them), 2 + g the energy of group g.  Every
// addition to a sample's energy goes to the total plane as it always did and to the plane of exactly ONE group: the group of the instance a light vertex or
// a light-sample ray hit, the environment's group for an environment vertex and for an environment ray that escapes.  Nothing is multiplied by zero.
//
// A light-sample item: group g's share is the sum, in ray order, of the contributions of the rays that belong to g, divided by light_samples — the rule of
// stage_shadow_item applied to each group's own terms.  A ray's contribution is folded into the accumulator of its group alone; the other accumulators are
// left as they are (lg_item_fold: a select over a compile-time index, so the eight accumulators are registers and no array is indexed at run time).  The group
// is that of the closest hit's instance when that hit is a light, the environment's otherwise.  The ray loop itself is routed_shadow_item (pt_routed_rules.h).
//
// The mix: out_c(p) = fold over g ascending of acc_c = acc_c + ((M[g][c][0] * X_g + M[g][c][1] * Y_g) + M[g][c][2] * Z_g), from acc_c = 0.0f; w = 0.
#ifndef PT_LIGHT_GROUP_RULES_H
#define PT_LIGHT_GROUP_RULES_H
#include "pt_routed_rules.h"

namespace ptd {

constexpr uint32_t LG_MAX_GROUPS = 8;    // PT_LIGHT_GROUPS_MAX of the header
constexpr uint32_t LG_FIRST_PLANE = 2;   // behind the total and the wavelength samples

// What a group render's vertex and light-sample forms are given: one byte per instance (device memory in the kernels), the environment's group, G.
struct LightGroupTable { const uint8_t* instance_group; uint32_t environment_group, group_count; };

PT_HD uint32_t lg_plane(uint32_t group) { return LG_FIRST_PLANE + group; }
PT_HD uint32_t lg_planes(uint32_t group_count) { return LG_FIRST_PLANE + group_count; }   // planes of a group render's energy buffer
// the group of a closest hit (a Hit's instance word, certificates' bits and all), or of the environment where nothing was hit
PT_HD uint32_t lg_hit_group(const SceneView& s, const LightGroupTable& t, bool valid, uint32_t instance_word) {
    return valid ? (uint32_t)t.instance_group[hit_instance_index(s, instance_word)] : t.environment_group;
}

// A vertex' energy addition (k_shade's `energy[slot] += out.energy_add[0]`, which the caller has made): the same addition to the plane of the vertex' group.
PT_HD void lg_add_vertex(const SceneView& s, const LightGroupTable& t, const Hit& hit, float add, float* energy, uint32_t energy_stride, uint32_t slot) {
    energy[(size_t)lg_plane(lg_hit_group(s, t, hit.valid, hit.instance)) * energy_stride + slot] += add;
}

PT_HD void lg_item_clear(float (&sums)[LG_MAX_GROUPS]) {
#pragma unroll
    for (uint32_t g = 0; g < LG_MAX_GROUPS; ++g) sums[g] = 0.0f;
}
PT_HD void lg_item_fold(float (&sums)[LG_MAX_GROUPS], uint32_t group, float contribution) {
#pragma unroll
    for (uint32_t g = 0; g < LG_MAX_GROUPS; ++g) sums[g] = group == g ? sums[g] + contribution : sums[g];
}
PT_HD void lg_item_add(const float (&sums)[LG_MAX_GROUPS], const LightGroupTable& t, uint32_t light_samples, float* energy, uint32_t energy_stride, uint32_t slot) {
#pragma unroll
    for (uint32_t g = 0; g < LG_MAX_GROUPS; ++g)
        if (g < t.group_count) energy[(size_t)lg_plane(g) * energy_stride + slot] += sums[g] / (float)light_samples;
}

// Light groups: the plane of the group of the instance a light vertex or a light-sample ray hit, the environment's group otherwise (the rules above).
struct GroupRouter {
    LightGroupTable t;
    typedef LightGroupTable Arg;
    PT_ROUTER_FN Arg arg() const { return t; }
    struct Vertex {};
    struct Item { float sums[LG_MAX_GROUPS]; };
    PT_ROUTER_FN Vertex vertex(const SceneView&, uint32_t, uint32_t, const Hit&) const { return Vertex{}; }
    PT_ROUTER_FN void ray(Vertex&, const Hit&, F3, uint32_t, F3) const {}
    PT_ROUTER_FN void add_vertex(const SceneView& s, const Vertex&, const Hit& hit, float add, float* energy, uint32_t energy_stride, uint32_t slot) const {
        lg_add_vertex(s, t, hit, add, energy, energy_stride, slot);
    }
    PT_ROUTER_FN void leave(const Vertex&, const Hit&, F3, bool, F3, uint32_t) const {}
    PT_ROUTER_FN Item item(uint32_t) const { Item it; lg_item_clear(it.sums); return it; }
    // (a ray that adds 0.0f adds it to the environment's group, which changes no sum)
    PT_ROUTER_FN void fold(const SceneView& s, Item& it, uint32_t, bool lit, uint32_t lit_instance, float c) const {
        lg_item_fold(it.sums, lit ? lg_hit_group(s, t, true, lit_instance) : t.environment_group, c);
    }
    PT_ROUTER_FN void add(const Item& it, uint32_t light_samples, float* energy, uint32_t energy_stride, uint32_t slot) const {
        lg_item_add(it.sums, t, light_samples, energy, energy_stride, slot);
    }
};

// One light-sample item of a group render by its earlier name and arguments: the previous revision's emulation sources compile against this header
template <int TRAV = PT_TRAV_ANY>
PT_HD void lg_shadow_item(const SceneView& s, const LightGroupTable& t, uint32_t light_samples, const Queue& shadow, uint32_t item, float* energy, uint32_t energy_stride) {
    routed_shadow_item<TRAV>(s, GroupRouter{t}, light_samples, shadow, item, energy, energy_stride);
}

// Group g's film pixel from group g's plane: stage_accumulate_pixel as it is, with the wavelength samples read where every render keeps them.
PT_HD void lg_accumulate_pixel(const RenderParams& rp, const float* energy, uint32_t group, uint32_t p, uint32_t pixel, float* film_px) {
    stage_accumulate_pixel<1>(rp, energy + (size_t)lg_plane(group) * rp.energy_stride, p, pixel, film_px, nullptr, energy + rp.energy_stride);
}

// The finish of an adaptive group render (pt_render_adaptive_light_groups): a group film pixel holds running sums, as the film does, until each pixel is divided
// by its own count — k_adaptive_finish's rule: x / (float)n per channel, w = 0, and a pixel of count 0 is left alone.
PT_HD void lg_adaptive_finish_pixel(uint32_t count, float* film_px) {
    if (count == 0u) return;
    const float c = (float)count;
    film_px[0] = film_px[0] / c; film_px[1] = film_px[1] / c; film_px[2] = film_px[2] / c; film_px[3] = 0.0f;
}

// The mix of one pixel.  load(g, &x, &y, &z): group g's film pixel; m: G x 9 floats, row-major 3 x 3 per group.
template <typename Load>
PT_HD void lg_mix_pixel(uint32_t group_count, const float* m, Load&& load, float* out_xyzw) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (uint32_t g = 0; g < group_count; ++g) {
        float x, y, z;
        load(g, &x, &y, &z);
        const float* r = m + 9u * g;
        a0 = a0 + ((r[0] * x + r[1] * y) + r[2] * z);
        a1 = a1 + ((r[3] * x + r[4] * y) + r[5] * z);
        a2 = a2 + ((r[6] * x + r[7] * y) + r[8] * z);
    }
    out_xyzw[0] = a0; out_xyzw[1] = a1; out_xyzw[2] = a2; out_xyzw[3] = 0.0f;
}

}  // namespace ptd
#endif
