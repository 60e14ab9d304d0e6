// pt_guides_chain_rules.h — the rules of the denoiser guides that follow specular chains (include/pt_denoise.h pt_render_guides_chain, DESIGN.md
// section 13 "Specular chains") as PT_HD functions that the engine's step kernel (pt_guides_chain.hip) and the host emulation of the tests
// (tests/host_emulation/ptemu_guides_chain.cpp) compile from the same text.  A guide sample starts as the camera ray of (pixel, k) and walks on through
// every mirror-like vertex — a passthrough boundary, a GGX material with alpha <= alpha_max — until it meets anything else, misses, or has followed
// max_chain vertices; the guides are taken there, with the path length where the first-hit distance stood.  The walk draws no random number: at a
// dielectric it always refracts (total internal reflection reflects), at a metal it reflects, both about the geometric normal.  The vector arithmetic
// is the path walk's own (stage_medium_surface, material_sample_p), so every value is an f32 evaluated in the order written; a numpy restatement
// (tests/test_guides_chain.py) gets it bit for bit.
#ifndef PT_GUIDES_CHAIN_RULES_H
#define PT_GUIDES_CHAIN_RULES_H
#include "pt_denoise_rules.h"
#include "pt_device.h"

namespace ptd {

enum { DN_CHAIN_MAX = 16 };
#define DN_CHAIN_DEFAULT_ALPHA_MAX 0.01f   /* between the material library's smooth GGX materials (alpha <= 0.004) and its rough ones (>= 0.02) */

// the material scalars the walk looks at (material_prepare's kind, metallic, alpha, ei, eo)
struct DnChainMaterial { uint32_t kind; int metallic; float alpha, ei, eo; };
struct DnChainNext { F3 wo, o, d; };

// whether the chain goes on through vertex v, whose hit carries `material_id`: an ordinary material (no light, not the camera), passthrough or smooth GGX,
// and the cap not reached
PT_HD bool dn_chain_follows(uint32_t material_id, uint32_t kind, float alpha, float alpha_max, uint32_t v, uint32_t max_chain) {
    if (PT_MATERIAL_TAG(material_id) != (uint32_t)PT_TAG_MATERIAL) return false;
    if (!(kind == (uint32_t)PT_MATERIAL_PASSTHROUGH || (kind == (uint32_t)PT_MATERIAL_GGX && alpha <= alpha_max))) return false;
    return v < max_chain;
}

// The next ray from a specular vertex: the hit's point p and normal n, the arriving direction d.  False (nothing to follow: the vertex is terminal)
// when a component of the new origin or direction is not finite.
PT_HD bool dn_chain_next(const DnChainMaterial& m, F3 p, F3 n, F3 d, DnChainNext* out) {
    const Frame frame = frame_from_normal(n);
    const F3 wi = normalize(to_local(frame, neg(d)));
    const F3 up = f3(0.0f, 0.0f, 1.0f);
    F3 wo;
    if (m.kind == (uint32_t)PT_MATERIAL_PASSTHROUGH) wo = neg(wi);
    else if (m.metallic) wo = reflect(wi, up);
    else {
        // (the microfacet normal of the walk lies on wi's side — sample_wh flips it for a ray that arrives from inside — and so does its smooth limit here)
        const float eta_rel = 1.0f / ggx_eta_rel(m.eo, m.ei, wi);
        if (!refract(wi, wi.z < 0.0f ? f3(0.0f, 0.0f, -1.0f) : up, eta_rel, &wo)) wo = reflect(wi, up);
    }
    out->wo = wo;
    out->o = add(p, mul(mul(n, 0.001f), wo.z > 0.0f ? 1.0f : -1.0f));
    out->d = normalize(to_world(frame, wo));
    return pt_isfinite(out->o.x) && pt_isfinite(out->o.y) && pt_isfinite(out->o.z) && pt_isfinite(out->d.x) && pt_isfinite(out->d.y) && pt_isfinite(out->d.z);
}

// One vertex of the chain at a valid hit.  Returns true and the next ray when the chain goes on; false when the vertex is terminal.
PT_HD bool dn_chain_vertex(const SceneView& s, uint32_t material_count, uint32_t material_id, F3 p, F3 n, float u, float v, F3 d, float lambda, float alpha_max,
                           uint32_t vertex, uint32_t max_chain, DnChainNext* out) {
    if (vertex >= max_chain || PT_MATERIAL_TAG(material_id) != (uint32_t)PT_TAG_MATERIAL || PT_MATERIAL_INDEX(material_id) >= material_count) return false;
    const uint32_t m = material_record(s, material_id);
    const uint32_t kind = bu(s, m + PT_MAT_KIND);
    if (!dn_chain_follows(material_id, kind, kind == (uint32_t)PT_MATERIAL_GGX ? bf(s, m + PT_MAT_ALPHA) : 0.0f, alpha_max, vertex, max_chain)) return false;
    const MatEval e = material_prepare(s, m, lambda, u, v);
    const DnChainMaterial cm{e.kind, e.metallic ? 1 : 0, e.alpha, e.ei, e.eo};
    return dn_chain_next(cm, p, n, d, out);
}

}  // namespace ptd
#endif
