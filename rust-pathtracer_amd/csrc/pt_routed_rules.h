// pt_routed_rules.h — a routed render (light groups; path passes, section 17): the FULL vertex form and the general light-sample form at
// one wavelength, unfused, no live list, whose every energy addition also goes to ONE more plane of the energy buffer.  Which plane is the router's business, a
// small struct the kernels (pt_kern_routed.hip) take by value; everything else is the two lane bodies below, PT_HD functions that the kernels and the host
// emulation of the tests (tests/host_emulation/ptemu_routed_pass.h) both compile: one text, so they agree bit for bit.  All f32, no contraction, in the order
// written.  Nothing here asks which router it serves: GroupRouter is in pt_light_group_rules.h, PassRouter in pt_path_pass_rules.h, each beside its rules.
//
// A router (Arg and arg(): what it is made of, the form in which it crosses a kernel launch — as an argument of its own, so that a pointer can be __restrict__):
//   Vertex vertex(s, bounce, slot, hit)                        what it knows in front of a vertex
//   void ray(v, hit, in_d, l, ray_d)                           light-sample ray l of the vertex' item was made
//   void add_vertex(s, v, hit, add, energy, stride, slot)      the vertex' own addition (made to the total plane by the caller): to its plane
//   void leave(v, hit, in_d, survives, next_d, slot)           behind the vertex
//   Item item(slot)                                            the sums of a light-sample item, cleared
//   void fold(s, item, l, lit, lit_instance, c)                ray l contributed c; lit: its closest hit is a light, of that instance word
//   void add(item, light_samples, energy, stride, slot)        the item's sums, each / light_samples, to their planes
#ifndef PT_ROUTED_RULES_H
#define PT_ROUTED_RULES_H
#include "pt_stages.h"

// PT_HD for a router's member functions: PT_HD's host form is `static inline`, which would make a member static
#if defined(__HIPCC__)
#define PT_ROUTER_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PT_ROUTER_FN inline
#endif

namespace ptd {

// One vertex of a routed render, the lane body of the vertex kernel: stage_shade's FULL form with the item's rays stored at position `ipos` of `shadow`, the
// item's head words, the addition to the total plane and to the router's.  `pv`: the path record with its slot's marks cleared; `wants_item`:
// shade_wants_item(s, rp, hit), for which the caller has reserved `ipos`; on_item(v, hit): called for a vertex that wants an item, behind its rays.
template <typename Router, typename OnItem>
PT_HD ShadeOutT<1> routed_vertex(const SceneView& s, const RenderParams& rp, const Router& router, uint32_t bounce, const PathVertexT<1>& pv, const Hit& hit, uint32_t pixel,
                                 bool wants_item, const Queue& shadow, uint32_t ipos, float* energy, OnItem&& on_item) {
    typename Router::Vertex v = router.vertex(s, bounce, pv.slot, hit);
    const ShadeOutT<1> out = stage_shade<1, true, true>(s, rp, bounce, pv, hit, pixel, [&](uint32_t l, const ShadowRayT<1>& ray) {
        store_shadow_ray<1>(shadow, ipos, l, ray);
        router.ray(v, hit, pv.d, l, ray.d);
    });
    if (wants_item) {
        qsu(shadow, Layout<1>::sh_slot, ipos, pv.slot); qsu(shadow, Layout<1>::sh_flags, ipos, out.env_mask);
        qsf(shadow, Layout<1>::sh_lambda, ipos, pv.lambda);
        if (!out.has_item) clear_shadow_item<1>(shadow, ipos, rp.light_samples);
        on_item(v, hit);
    }
    if (out.add_energy) {
        energy[pv.slot] += out.energy_add[0];
        router.add_vertex(s, v, hit, out.energy_add[0], energy, rp.energy_stride, pv.slot);
    }
    router.leave(v, hit, pv.d, out.survives, out.next.d, pv.slot);
    return out;
}

// One light-sample item of a routed render: stage_shadow_item<1, TRAV, true> — the same rays, searches and total — with every ray's contribution folded by the
// router too, in ray order, and the router's sums added behind the total (the rule of stage_shadow_item applied to each plane's own terms).
template <int TRAV = PT_TRAV_ANY, typename Router>
PT_HD void routed_shadow_item(const SceneView& s, const Router& router, uint32_t light_samples, const Queue& shadow, uint32_t item, float* energy, uint32_t energy_stride) {
    const bool marks = TRAV != PT_TRAV_SWEEP && scene_has_certificates(s);
    const uint32_t slot = qu(shadow, Layout<1>::sh_slot, item), flags = qu(shadow, Layout<1>::sh_flags, item);
    const float lambda0 = qf(shadow, Layout<1>::sh_lambda, item);
    float lc = 0.0f;
    typename Router::Item sums = router.item(slot);
    for (uint32_t l = 0; l < light_samples; ++l) {
        ShadowRayT<1> ray;
        if (!load_shadow_ray<1, false>(shadow, item, l, &ray)) continue;
        const bool env = ((flags >> l) & 1u) != 0u;
        const uint32_t skip_inst = (marks && ((flags >> (8u + l)) & 1u) != 0u) ? flags >> 16 : 0xffffffffu;
        float c[1] = {0.0f};
        bool lit = false;
        uint32_t lit_instance = 0u;
        float bound = PT_INF; int stop = PT_STOP_NONE;
        uint32_t light = 0xffffffffu;
        bool search = true;
        if (env) stop = shadow_env_stop(s);
        else search = shadow_light_bound(s, ray.o, ray.d, &bound, &stop, &light);
        if (search) {
            Hit sh;
            const bool hit = world_hit<TRAV, true>(s, ray.o, ray.d, &sh, bound, stop, light, bound, skip_inst);
            shadow_ray_contribution<1>(s, [&](int) { return lambda0; }, ray, env, hit, sh, c);
            lit = !env && hit && PT_MATERIAL_TAG(sh.material) == PT_TAG_LIGHT;
            lit_instance = lit ? sh.instance : 0u;   // (a miss leaves sh as it was)
        }
        lc += c[0];
        router.fold(s, sums, l, lit, lit_instance, c[0]);
    }
    energy[slot] += lc / (float)light_samples;
    router.add(sums, light_samples, energy, energy_stride, slot);
}

}  // namespace ptd
#endif
