// pt_device.h — per-lane device logic of the HIP path tracer (gfx950).
//
// Everything a single lane computes: scene-blob accessors, ray/primitive tests with the reference's
// interval rules, the two-level skip-link BVH walk, spectral curve evaluation, the four materials,
// light sampling and the thin-lens camera.  The kernels in pt_kernels.hip are thin: they stage the
// blob into LDS, move SoA state between HBM and registers, call these functions, and compact queues.
//
// All functions are __host__ __device__ so tests can run the same lane logic on the CPU
// (tests/host_emulation) before it is trusted on the GPU; the shipped library only uses the device side.
//
// Arithmetic rules (include/pt_numerics.h): no contraction, IEEE division and sqrt, transcendental
// functions only from pt_numerics.h, expressions written in the operation order documented in
// DESIGN.md "numeric contract" so that path decisions match the CPU oracle bit for bit.
//
// Reference citations are relative to /root/reference (gillett-hernandez/rust-pathtracer @ 2024_08_07).
#ifndef PT_DEVICE_H
#define PT_DEVICE_H

#include "../../include/pt_api.h"
#include "../../include/pt_numerics.h"
#include "pt_blob.h"

// Predicates in this header are combined with `&` and `|` ON PURPOSE: `&&` / `||` of comparisons compile to a branch around the next comparison — three scalar
// instructions each on a unit the kernels were bound by ("The scalar unit").  No operand has a side effect, so the two spellings mean the same.
#if defined(__clang__)
#pragma clang diagnostic ignored "-Wbitwise-instead-of-logical"
#endif

#ifndef PT_CURVE_CELLS
#define PT_CURVE_CELLS 1   /* tabulated curves: the knot index from the curve's cell table (round 5); 0 = the binary search everywhere */
#endif
#ifndef PT_GROUP_WAVE_MASKS
#define PT_GROUP_WAVE_MASKS 0   /* 1 = the grouped mesh sweep's group boxes decided as wave masks (round 5 experiment 14: C3 k_extend_parked -1.8 %, frame within noise; off) */
#endif
#ifndef PT_GROUP_WALK_BOX
#define PT_GROUP_WALK_BOX 1   /* the grouped mesh sweep's per-lane leaf boxes through walk_box (round 5); 0 = aabb_classify + a loop over the undecided */
#endif

// Optional instrumentation for host-side experiments (tools/traversal_stats.cpp); compiled out everywhere else.
#ifndef PT_STAT
#define PT_STAT(counter)
#endif
#ifndef PT_STAT_EVENT
#define PT_STAT_EVENT(code)
#endif
#ifndef PT_STAT_RAY
#define PT_STAT_RAY(o, d)
#endif
#ifndef PT_STAT_WALK
#define PT_STAT_WALK(lo, ld, bound, closest, stop)   /* a mesh walk begins (tools/light_walks.cpp): the ray in the instance's own space, its bound, the closest hit so far */
#define PT_STAT_WALK_END(over)                       /* ... and ends: whether the search is over (an early stop) */
#endif
#ifndef PT_STAT_FIRST_GROUP
#define PT_STAT_FIRST_GROUP(found, spoiled)          /* the grouped sweep tried an inside ray's farthest-reaching group first: with what result */
#endif
#ifndef PT_STAT_INSIDE_STOP
#define PT_STAT_INSIDE_STOP()                        /* a sweep ended by mesh_walk's `inside` rule (tests/host_emulation counts them) */
#endif

// Wave-level helpers: device code sees the wave, the host emulation one lane at a time.
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_KEEP_BRANCH() asm volatile("" ::: "memory")   /* inside a rarely taken block: the compiler must not turn it into selects */
#define PT_KEEP_BRANCH_NOFENCE() asm volatile("")   /* the same for a block that IS taken often: no memory clobber, the loads and stores around it schedule freely */
#define PT_WAVE_ANY(x) (__builtin_amdgcn_ballot_w64(x) != 0)
#define PT_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))  /* a value every lane of the wave holds */
#define PT_WAVE_ACTIVE(host_value) ((uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true)))  /* the lanes that execute this line */
#define PT_WAVE_BALLOT(x) ((unsigned long long)__builtin_amdgcn_ballot_w64(x))
#define PT_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b))   /* the two values exist here, in vector registers: their loads are not sunk past this point */
#define PT_WAVE_MEMBER(mask) (__builtin_amdgcn_inverse_ballot_w64(mask))   /* whether this lane's bit is set in a wave-uniform mask: the mask itself as the lane predicate, no instruction */
#define PT_WAVE_RANK(mask) ((uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)((mask) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)(mask), 0u)))  /* set bits of `mask` below this lane */
#define PT_WAVE_READ(x, lane) ((uint32_t)__builtin_amdgcn_readlane((int)(x), (int)(lane)))   /* lane's value of a 32-bit x, in every lane (a scalar) */
#else
#define PT_KEEP_BRANCH()
#define PT_KEEP_BRANCH_NOFENCE()
#define PT_WAVE_ANY(x) (x)
#define PT_UNIFORM(x) (x)
#define PT_WAVE_ACTIVE(host_value) (host_value)
#define PT_WAVE_BALLOT(x) ((x) ? 1ull : 0ull)
#define PT_PIN2(a, b)
#define PT_WAVE_MEMBER(mask) (((mask) & 1ull) != 0ull)
#define PT_WAVE_RANK(mask) 0u
#define PT_WAVE_READ(x, lane) ((void)(lane), (uint32_t)(x))
#endif

// A loop the compiler must keep rolled (the per-wavelength loops of the hero variant: four inlined copies of a curve evaluation cost
// registers and instruction cache for nothing).
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_ROLLED _Pragma("clang loop unroll(disable)")
#else
#define PT_ROLLED
#endif

namespace ptd {

// Element k of a small per-wavelength array held in registers, k a loop counter of a ROLLED loop: addressing the array with k would send
// it — and the struct around it — to scratch memory (k_shade<4> kept 304 B per lane there, k_shadow<4> 44 B).  k is wave-uniform, so a chain
// of N - 1 selects on scalar conditions reads it and N selects write it; every index below is a constant after unrolling.
// (Written out, not as loops over i, and every element passed through an empty asm statement: left to itself the optimiser folds the
// chain of selects over loads from one array back into a single load at a[k] — the very indexed access this is here to avoid.)
PT_HD float pl_opaque(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}
template <int N> PT_HD float pl_get(const float (&a)[N], int k) {
    static_assert(N >= 1 && N <= 4, "per-wavelength arrays hold 1 or 4 values");
    if (N == 1) return a[0];
    float r = pl_opaque(a[0]);
    if (N > 1) r = (k == 1) ? pl_opaque(a[1 % N]) : r;
    if (N > 2) r = (k == 2) ? pl_opaque(a[2 % N]) : r;
    if (N > 3) r = (k == 3) ? pl_opaque(a[3 % N]) : r;
    return r;
}
template <int N> PT_HD void pl_set(float (&a)[N], int k, float x) {
    static_assert(N >= 1 && N <= 4, "per-wavelength arrays hold 1 or 4 values");
    if (N == 1) { a[0] = x; return; }
    a[0] = (k == 0) ? x : pl_opaque(a[0]);
    if (N > 1) a[1 % N] = (k == 1) ? x : pl_opaque(a[1 % N]);
    if (N > 2) a[2 % N] = (k == 2) ? x : pl_opaque(a[2 % N]);
    if (N > 3) a[3 % N] = (k == 3) ? x : pl_opaque(a[3 % N]);
}

template <int V> struct IntC { static constexpr int value = V; };   // a compile-time integer as a value (generic lambdas)
struct F3 { float x, y, z; };
struct alignas(16) F4 { float x, y, z, w; };

PT_HD F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_HD F3 add(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_HD F3 sub(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_HD F3 neg(F3 a) { return f3(-a.x, -a.y, -a.z); }
PT_HD F3 mul(F3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
PT_HD F3 divs(F3 a, float s) { return f3(a.x / s, a.y / s, a.z / s); }
PT_HD float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PT_HD F3 cross(F3 a, F3 b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
PT_HD float norm(F3 a) { return pt_sqrt(dot(a, a)); }
PT_HD F3 normalize(F3 a) { return divs(a, norm(a)); }

// ---------------------------------------------------------------- blob access
struct SceneView {
    const uint32_t* w;  // core section of the blob (everything but mesh data): LDS copy or HBM
    const float* tex;   // texture texels, HBM
    const uint32_t* m;  // mesh-data section (BVH nodes, triangles, normals, leaf lists; offsets relative to it): LDS copy or HBM
    // What the scene is known NOT to hold (PT_SCENE_*): a kernel form sets it from a template constant, and after inlining the branches
    // that depend on it fold away — registers and code size change, results do not (a scene that does hold the thing never gets the form).
    uint32_t lacks = 0u;
    // The marginal tables of the importance map (interleaved cmf / pdf pairs and their guide) staged in LDS by the FULL vertex form (k_shade, stage_marginal): every
    // environment sample starts with a search of these 12 KB.  marg_words = 0: not staged (every other kernel, the host): the texture memory's copy is read.
    const float* marg = nullptr;
    uint32_t marg_words = 0u, marg_base = 0u, marg_guide = 0u;   // floats staged from tex + marg_base; the guide's offset inside them (0: none)
    // PT_FLAG_CONVEX of the header (round 6: some instance carries a convex-body certificate), read ONCE per kernel from the blob's HBM copy through the kernel's scalar
    // argument (stage_scene): a scalar register, so that the certificate code in hit_record and stage_shade stands behind scalar branches and costs a scene without
    // certificates no vector instruction (measured before this: 2-4 % of the vertex kernels of every such scene, profiles/r6g_ab_r5.txt).
    uint32_t certs = 0u;
};
#define PT_SCENE_NO_XF 1u   /* no instance carries a transform (the Cornell box): instance_local_ray and the hit record's way back are identities */
#define PT_SCENE_NO_LIGHTS 2u /* the light list is empty (an environment is the only emitter: hdri_test): no light vertex, no light to sample */
#define PT_SCENE_NO_CERTS 4u  /* no instance carries a convex-body certificate (PT_FLAG_CONVEX clear): the certificate code of hit_record and stage_shade is compiled out.  Every
                                 vertex-kernel form has this bit but the two made for such scenes (k_shade NO_ENV / FULL "with certificates", pt_kern_shade.hip) — measured: with the
                                 code present behind scalar branches the fused and lean forms still lost 2 % (registers, layout: profiles/r6h_ab_r5b.txt) */
#define PT_SCENE_NO_MESH_LIGHTS 8u /* no light-list entry is an emissive mesh face (PT_HDR_LIGHT_FACE_OFF = 0): the face's sampler, its pdf and its area in the hit record are
                                      compiled out.  Every kernel form carries this bit but the few the engine gives a scene with emissive faces (pt_kern_*.hip) */
PT_HD uint32_t bu(const SceneView& s, uint32_t off) { return s.w[off]; }
#if defined(__HIP_DEVICE_COMPILE__)
PT_HD bool scene_has_certificates(const SceneView& s) { return !(s.lacks & PT_SCENE_NO_CERTS) && s.certs != 0u; }
#else
PT_HD bool scene_has_certificates(const SceneView& s) { return (s.w[21] & 2048u) != 0u; }   // (the host emulation builds its views by hand: PT_HDR_FLAGS & PT_FLAG_CONVEX, pt_blob.h)
#endif
// The instance a hit lies on: in a scene with certificates the hit's instance word also carries its face's claims (hit_record)
PT_HD uint32_t hit_instance_index(const SceneView& s, uint32_t instance_word) { return scene_has_certificates(s) ? instance_word & PT_HIT_INDEX_MASK : instance_word; }
PT_HD float bf(const SceneView& s, uint32_t off) { return pt_u2f(s.w[off]); }
PT_HD F4 bf4(const SceneView& s, uint32_t off) { return *reinterpret_cast<const F4*>(s.w + off); }
PT_HD F3 bf3(const SceneView& s, uint32_t off) { return f3(bf(s, off), bf(s, off + 1), bf(s, off + 2)); }
PT_HD uint32_t mu(const SceneView& s, uint32_t off) { return s.m[off]; }
PT_HD F4 mf4(const SceneView& s, uint32_t off) { return *reinterpret_cast<const F4*>(s.m + off); }
PT_HD bool instance_is_transformed(const SceneView& s, uint32_t inst) { return !(s.lacks & PT_SCENE_NO_XF) && (bu(s, inst + PT_INST_FLAGS) & 1u) != 0u; }
PT_HD bool sweep_leaf_transformed(const SceneView& s, uint32_t kf) { return !(s.lacks & PT_SCENE_NO_XF) && (kf & 0x200u) != 0u; }   // (kf: the sweep table's kind-and-flags word)

// TangentFrame::from_normal (math crate): Duff et al. 2017.
struct Frame { F3 t, b, n; };
PT_HD Frame frame_from_normal(F3 n) {
    float sign = (pt_f2u(n.z) & 0x80000000u) ? -1.0f : 1.0f;
    float a = -1.0f / (sign + n.z);
    float b = n.x * n.y * a;
    Frame f;
    f.t = f3(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
    f.b = f3(b, sign + n.y * n.y * a, -n.y);
    f.n = n;
    return f;
}
PT_HD F3 to_world(const Frame& f, F3 v) { return add(add(mul(f.t, v.x), mul(f.b, v.y)), mul(f.n, v.z)); }
PT_HD F3 to_local(const Frame& f, F3 v) { return f3(dot(f.t, v), dot(f.b, v), dot(f.n, v)); }

// rows 0..2 of a 4x4 at word offset `m`
PT_HD F3 xf_point(const SceneView& s, uint32_t m, F3 p) {
    return f3(bf(s, m + 0) * p.x + bf(s, m + 1) * p.y + bf(s, m + 2) * p.z + bf(s, m + 3),
              bf(s, m + 4) * p.x + bf(s, m + 5) * p.y + bf(s, m + 6) * p.z + bf(s, m + 7),
              bf(s, m + 8) * p.x + bf(s, m + 9) * p.y + bf(s, m + 10) * p.z + bf(s, m + 11));
}
PT_HD F3 xf_vec(const SceneView& s, uint32_t m, F3 v) {
    return f3(bf(s, m + 0) * v.x + bf(s, m + 1) * v.y + bf(s, m + 2) * v.z,
              bf(s, m + 4) * v.x + bf(s, m + 5) * v.y + bf(s, m + 6) * v.z,
              bf(s, m + 8) * v.x + bf(s, m + 9) * v.y + bf(s, m + 10) * v.z);
}
PT_HD F3 xf_vec_transposed(const SceneView& s, uint32_t m, F3 v) {
    return f3(bf(s, m + 0) * v.x + bf(s, m + 4) * v.y + bf(s, m + 8) * v.z,
              bf(s, m + 1) * v.x + bf(s, m + 5) * v.y + bf(s, m + 9) * v.z,
              bf(s, m + 2) * v.x + bf(s, m + 6) * v.y + bf(s, m + 10) * v.z);
}

// ---------------------------------------------------------------- spectral curves (math::curves::Curve::evaluate)
PT_HD float gaussianf32(float x, float alpha, float mu, float s1, float s2) {
    float t = (x - mu) / (x < mu ? s1 : s2);
    return alpha * pt_exp(-(t * t) / 2.0f);
}
PT_HD float blackbody(float temperature, float lambda_nm) {
    float l = lambda_nm * 1e-9f;
    float l2 = l * l;
    float l5 = l2 * l2 * l;
    return (1.0f / l5) * 1.1910429723971884140794892e-29f /
           (pt_exp(1.438777085924334052222404423195819240925e-2f / (l * temperature)) - 1.0f);
}
PT_HD float interp(uint32_t mode, float t, float left, float right) {
    if (mode == PT_INTERP_LINEAR) return (1.0f - t) * left + t * right;
    if (mode == PT_INTERP_NEAREST) return t < 0.5f ? left : right;
    float t2 = 2.0f * t;
    float omt = 1.0f - t;
    float h00 = (1.0f + t2) * omt * omt;
    float h01 = t * t * (3.0f - t2);
    return h00 * left + h01 * right;
}
PT_HD float curve_eval(const SceneView& s, uint32_t c, float lambda) {
    uint32_t kind = bu(s, c), mode = bu(s, c + 1);
    float p0 = bf(s, c + 2), p1 = bf(s, c + 3);
    uint32_t d = bu(s, c + 4), n = bu(s, c + 5);
    switch (kind) {
        case PT_CURVE_LINEAR: {
            if (lambda < p0 || lambda > p1) return 0.0f;
            float step = (p1 - p0) / (float)n;
            float fi = (lambda - p0) / step;
            uint32_t index = (fi >= 0.0f) ? (uint32_t)fi : 0u;
            if (index >= n) index = n - 1;
            float left = bf(s, d + index);
            if (index + 1 >= n) return left;
            float right = bf(s, d + index + 1);
            float t = (lambda - (p0 + (float)index * step)) / step;
            return interp(mode, t, left, right);
        }
        case PT_CURVE_TABULATED: {
            uint32_t lo = 0, hi = n;
            const uint32_t grid = PT_CURVE_CELLS ? bu(s, c + PT_CURVE_GRID) : 0u;
            if (grid != 0u) {
                // the first knot that is not below lambda — the binary search's answer — found from the cell table (pt_scene_host.cpp): every knot in a lower cell
                // is below lambda, the walk passes the knots of lambda's own cell
                const float fi = (lambda - bf(s, d)) * bf(s, c + PT_CURVE_GRID_INV);
                const float top = (float)(grid >> 24);
                const uint32_t g = fi >= 0.0f ? (uint32_t)(fi < top ? fi : top) : 0u;
                lo = (bu(s, (grid & 0xffffffu) + (g >> 2)) >> ((g & 3u) * 8u)) & 0xffu;
                while (lo < n && bf(s, d + 2 * lo) < lambda) ++lo;
            } else
            while (lo < hi) {
                uint32_t mid = lo + (hi - lo) / 2;
                if (bf(s, d + 2 * mid) < lambda) lo = mid + 1; else hi = mid;
            }
            if (lo == n) return bf(s, d + 2 * (n - 1) + 1);
            if (lo == 0) return bf(s, d + 1);
            float lx = bf(s, d + 2 * (lo - 1)), ly = bf(s, d + 2 * (lo - 1) + 1);
            float rx = bf(s, d + 2 * lo), ry = bf(s, d + 2 * lo + 1);
            float t = (lambda - lx) / (rx - lx);
            return interp(mode, t, ly, ry);
        }
        case PT_CURVE_CAUCHY: return p0 + p1 / (lambda * lambda);
        case PT_CURVE_EXPONENTIAL: {
            float val = 0.0f;
            for (uint32_t i = 0; i < n; ++i)
                val += gaussianf32(lambda, bf(s, d + 4 * i + 3), bf(s, d + 4 * i), bf(s, d + 4 * i + 1), bf(s, d + 4 * i + 2));
            return val;
        }
        case PT_CURVE_INV_EXPONENTIAL: {
            float val = 1.0f;
            for (uint32_t i = 0; i < n; ++i)
                val -= gaussianf32(lambda, bf(s, d + 4 * i + 3), bf(s, d + 4 * i), bf(s, d + 4 * i + 1), bf(s, d + 4 * i + 2));
            return pt_max(val, 0.0f);
        }
        case PT_CURVE_BLACKBODY: {
            if (p1 == 0.0f) return blackbody(p0, lambda);
            return p1 * blackbody(p0, lambda) / blackbody(p0, 2.8977721e-3f / (p0 * 1e-9f));
        }
        case PT_CURVE_CONST: return pt_max(p0, 0.0f);
        default: return 0.0f;
    }
}

// TexStack::eval_at (src/texture.rs:258-265), nearest texel (src/vec2d.rs:34-42).  A layer's curves depend on the wavelength only:
// LayerCurves holds their values so that a caller evaluating one stack at many (u, v) of one wavelength evaluates them once.
struct LayerCurves { float c0, c1, c2, c3; };
PT_HD LayerCurves layer_curves(const SceneView& s, uint32_t l, float lambda) {
    LayerCurves c;
    c.c0 = curve_eval(s, bu(s, l + 1), lambda);
    c.c1 = c.c2 = c.c3 = 0.0f;
    if (bu(s, l) != PT_TEXTURE1) { c.c1 = curve_eval(s, bu(s, l + 2), lambda); c.c2 = curve_eval(s, bu(s, l + 3), lambda); c.c3 = curve_eval(s, bu(s, l + 4), lambda); }
    return c;
}
PT_HD float layer_eval(const SceneView& s, uint32_t l, const LayerCurves& c, float u, float v) {
    uint32_t kind = bu(s, l), w = bu(s, l + 5), h = bu(s, l + 6), toff = bu(s, l + 7);
    float cu = pt_clamp(u, 0.0f, 1.0f - PT_F32_EPSILON), cv = pt_clamp(v, 0.0f, 1.0f - PT_F32_EPSILON);
    uint32_t x = (uint32_t)(cu * (float)w), y = (uint32_t)(cv * (float)h);
#if defined(PT_EXP_TABLE_FOLD)
    if (h >= 64u * PT_EXP_TABLE_FOLD) y %= h / PT_EXP_TABLE_FOLD;   // (a TIMING experiment, never the product: see env_sample_uv)
#endif
    uint32_t idx = y * w + x;
    if (kind == PT_TEXTURE1) return c.c0 * s.tex[toff + idx];
    const float* t = s.tex + toff + 4u * idx;
    float e0 = c.c0 * t[0], e1 = c.c1 * t[1];
    float e2 = c.c2 * t[2], e3 = c.c3 * t[3];
    return (e0 + e1) + (e2 + e3);
}
PT_HD float texstack_eval(const SceneView& s, uint32_t ts, float lambda, float u, float v) {
    uint32_t layers = bu(s, ts);
    float energy = 0.0f;
    for (uint32_t i = 0; i < layers; ++i) {
        uint32_t l = ts + 1 + i * PT_LAYER_WORDS;
        energy += layer_eval(s, l, layer_curves(s, l, lambda), u, v);
    }
    return energy;
}

// ---------------------------------------------------------------- intersection
struct Hit {
    float t; F3 p, n; float u, v; uint32_t material, instance; bool valid;
};

// AABB::hit (src/aabb.rs:37-65) for the (t0, t1) = (0, inf) every caller on this path passes: slab test clipped
// against t >= 0 by the w lane (d.w = 0 -> tmin 0, tmax inf).  The second rejection test of the reference is
// implied by the first for these bounds.  Exact form: six IEEE divisions.
PT_HD bool aabb_hit_exact(F4 a, F4 b, F3 o, F3 d, float* entry) {
    float n0, x0, n1, x1, n2, x2;
    if (d.x == 0.0f) { n0 = 0.0f; x0 = PT_INF; } else { float p = (a.x - o.x) / d.x, q = (b.x - o.x) / d.x; n0 = __builtin_fminf(p, q); x0 = __builtin_fmaxf(p, q); }
    if (d.y == 0.0f) { n1 = 0.0f; x1 = PT_INF; } else { float p = (a.y - o.y) / d.y, q = (b.y - o.y) / d.y; n1 = __builtin_fminf(p, q); x1 = __builtin_fmaxf(p, q); }
    if (d.z == 0.0f) { n2 = 0.0f; x2 = PT_INF; } else { float p = (a.z - o.z) / d.z, q = (b.z - o.z) / d.z; n2 = __builtin_fminf(p, q); x2 = __builtin_fmaxf(p, q); }
    float tmin_max = __builtin_fmaxf(__builtin_fmaxf(n0, n1), __builtin_fmaxf(n2, 0.0f));
    float tmax_min = __builtin_fminf(__builtin_fminf(x0, x1), x2);
    *entry = tmin_max;
    return !(tmin_max > tmax_min);
}

// ---- filtered slab test ---------------------------------------------------------------------------------------
// The exact test costs ~100 VALU instructions per node (each IEEE f32 division is ~11).  Its *decision* can almost
// always be certified from approximate quotients: with r ~ 1/d (v_rcp_f32, <= 1 ulp) the products (c - o) * r are within
// 3e-7 relative of the correctly rounded quotients, so a comparison of two of them that is decided by more than
// PT_SLAB_EPS relative is decided the same way by the exact values.  Only comparisons too close to call fall back to
// the divisions.  hit <=> for every axis j: max(0, entry_i for i != j) <= exit_j (the i == j pairs hold by
// construction), which keeps zero-thickness boxes — every axis-aligned wall of the Cornell box — on the fast path.
// The returned decision is therefore always the exact one; `entry` may be the approximate entry distance.
#define PT_SLAB_EPS 4e-6f
#define PT_SLAB_TINY 1e-30f
PT_HD float fast_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
// p ~ (c - o) / d is evaluated as fma(c, r, -o*r): one instruction per slab plane.  Its absolute error is bounded by
// 2e-7 * (2 |o r| + |p|); the margin below uses PT_SLAB_EPS (4e-6) * (max_i |o_i r_i| + |entry| + |exit|), 10x that.
PT_HD float approx_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmaf(a, b, c);
#else
    return a * b + c;  // any approximation within the margin will do on the host
#endif
}
struct RayPrep { F3 o, d, r, nor; float base; bool fast; };
PT_HD RayPrep ray_prepare(F3 o, F3 d) {
    RayPrep p; p.o = o; p.d = d;
    float ax = pt_abs(d.x), ay = pt_abs(d.y), az = pt_abs(d.z);
    p.r = f3(d.x == 0.0f ? 0.0f : fast_rcp(d.x), d.y == 0.0f ? 0.0f : fast_rcp(d.y), d.z == 0.0f ? 0.0f : fast_rcp(d.z));
    p.nor = f3(-(o.x * p.r.x), -(o.y * p.r.y), -(o.z * p.r.z));
    float k = __builtin_fmaxf(__builtin_fmaxf(pt_abs(p.nor.x), pt_abs(p.nor.y)), pt_abs(p.nor.z));
    p.base = PT_SLAB_EPS * k + PT_SLAB_TINY;
    // reciprocals must be finite and the products must not overflow: |d| in (1e-18, 1e18) or exactly 0, finite origin
    // (`&`, `|`: comparisons combined as data — each `&&` / `||` here was compiled as a branch around the next comparison)
    bool okx = (ax == 0.0f) | ((ax > 1e-18f) & (ax < 1e18f)), oky = (ay == 0.0f) | ((ay > 1e-18f) & (ay < 1e18f)), okz = (az == 0.0f) | ((az > 1e-18f) & (az < 1e18f));
    bool oko = (pt_abs(o.x) < 1e18f) & (pt_abs(o.y) < 1e18f) & (pt_abs(o.z) < 1e18f);
    p.fast = okx & oky & okz & oko;
    return p;
}
PT_HD bool aabb_hit(F4 a, F4 b, const RayPrep& rp, float* entry) {
    PT_STAT(box_tests);
    if (rp.fast) {
        float n0, x0, n1, x1, n2, x2;
        bool z0 = rp.d.x == 0.0f, z1 = rp.d.y == 0.0f, z2 = rp.d.z == 0.0f;
        if (z0) { n0 = 0.0f; x0 = PT_INF; } else { float p = approx_fma(a.x, rp.r.x, rp.nor.x), q = approx_fma(b.x, rp.r.x, rp.nor.x); n0 = __builtin_fminf(p, q); x0 = __builtin_fmaxf(p, q); }
        if (z1) { n1 = 0.0f; x1 = PT_INF; } else { float p = approx_fma(a.y, rp.r.y, rp.nor.y), q = approx_fma(b.y, rp.r.y, rp.nor.y); n1 = __builtin_fminf(p, q); x1 = __builtin_fmaxf(p, q); }
        if (z2) { n2 = 0.0f; x2 = PT_INF; } else { float p = approx_fma(a.z, rp.r.z, rp.nor.z), q = approx_fma(b.z, rp.r.z, rp.nor.z); n2 = __builtin_fminf(p, q); x2 = __builtin_fmaxf(p, q); }
        float m0 = __builtin_fmaxf(__builtin_fmaxf(n1, n2), 0.0f), m1 = __builtin_fmaxf(__builtin_fmaxf(n0, n2), 0.0f), m2 = __builtin_fmaxf(__builtin_fmaxf(n0, n1), 0.0f);
        float e0 = approx_fma(PT_SLAB_EPS, m0 + pt_abs(x0), rp.base), e1 = approx_fma(PT_SLAB_EPS, m1 + pt_abs(x1), rp.base), e2 = approx_fma(PT_SLAB_EPS, m2 + pt_abs(x2), rp.base);
        bool miss = (!z0 && m0 > x0 + e0) || (!z1 && m1 > x1 + e1) || (!z2 && m2 > x2 + e2);
        if (miss) return false;
        bool hit = (z0 || m0 < x0 - e0) && (z1 || m1 < x1 - e1) && (z2 || m2 < x2 - e2);
        if (hit) { *entry = __builtin_fmaxf(m0, n0); return true; }
    }
    PT_STAT(box_exact);
    return aabb_hit_exact(a, b, rp.o, rp.d, entry);
}
// Conservative cull: a node whose (approximate or exact) entry distance exceeds the closest hit so far by more than a margin cannot
// contain a primitive whose computed hit is closer.  Primitives lie inside their boxes (except the reference's half-size Disk box,
// for which culling is switched off), but a computed t can fall short of the box.  A triangle's t is an average of its vertices'
// depths with same-sign weights, a rect's or disk's one division: a few ulp, margin 1e-5.  A sphere's comes out of -b - sqrt(b^2 - ac):
// for a grazing ray the cancellation under the root costs up to sqrt(2 eps) = 4.9e-4 of t, and for a ray that starts close to a big
// sphere the cancellation of -b against the root costs eps * |b|, which no margin relative to t covers.  So a box that holds a sphere
// is never culled: sphere instances in the sweep table, and the nodes of the top-level BVH flagged PT_NODE_NO_CULL by the host.
// (History: every box had margin 1e-5 until the GPU soak met a grazing ray — fuzz seed 101684, a light-sample ray bounded by its own
// sphere light culled the light; spheres then got a margin of 2e-3, which the second case above still defeats.)
PT_HD bool beyond(float entry, float closest, float base) { return entry > closest * 1.00001f + base; }
// ... and since round 6 a box that holds UNTRANSFORMED spheres is culled too, by a margin CERTIFIED from the quadratic's error (the round-5 verdict's item 3; before, a scene of
// many sphere lights — test_bokeh.toml — walked its top-level tree without any culling by the closest hit).  With u = 2^-24, D the distance from the ray's origin to a sphere's
// centre, r its radius: oc . d, oc . oc - r^2 and the discriminant b^2 - a c are each right to a few u (D + r)^2, so the computed root t solves a quadratic whose value AT t is
// off by F <= 40 u (D + r)^2: the computed hit point lies within eta = sqrt(F) = 1.55e-3 (D + r) of the sphere, hence inside the sphere's box grown by eta.  A ray the reference
// tests against the sphere enters the sphere's own box (its box test passed), and between entering the grown box and the box itself it travels at most the grown box's diagonal,
// 2 sqrt(3) (r + eta) <= 3.5 (r + eta): computed t >= box entry - 3.5 (r + eta).  An ancestor's entry is no later, and D <= entry + diagonal of the ancestor's box.  So a node
// whose entry distance exceeds the closest hit by m0 + K entry, m0 = 3.5 r_max + K (diagonal + r_max), K = 3.5 x 1.55e-3 = 5.4e-3 (PT_SPHERE_CULL_K), holds no sphere whose
// computed hit would be accepted.  m0 comes from the host per top-level node (pt_blob.h PT_HDR_TOP_MARGIN): 0 = no sphere below the node (the plain rule), +inf = never.
// (scene.big_sphere_light — radius 20 000 — gets m0 = 70 000: never culled in practice, as before.)
PT_HD bool beyond_sphere(float entry, float closest, float base, float m0) {
    return (m0 != 0.0f ? entry * (1.0f - (float)PT_SPHERE_CULL_K) : entry) > closest * 1.00001f + base + m0;
}

// The filtered test classifies: hit, miss, or too close to call (the caller settles it with aabb_hit_exact).  It requires rp.fast and
// no zero direction component.  A box of zero thickness along some axis (known per box on the host) takes the per-axis form of aabb_hit
// above; other boxes the plain comparison of max entry and min exit, whose approximation error is covered by the same margin.
// max(a, b, c, 0) and min(a, b, c) of slab distances: two / one instruction on the device (the compiler's own lowering of the fmaxf
// chain spends two more on quieting signalling NaNs that arithmetic results cannot be)
#if defined(__HIP_DEVICE_COMPILE__)
PT_HD float slab_entry(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, 0, %0" : "=&v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
PT_HD float slab_exit(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
PT_HD float pt_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
#else
PT_HD float pt_max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
PT_HD float slab_entry(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(a, b), c), 0.0f); }
PT_HD float slab_exit(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }
#endif
// The decision as two wave masks (the lanes that hit, the lanes too close to call).  A lane predicate that crosses a branch — even a wave-uniform one — is
// merged by the compiler with three scalar instructions per predicate and path (and-not exec, and exec, or); a ballot is the comparison's own result, and a
// wave mask crosses control flow as a plain scalar value.  The scalar unit is shared by the four SIMDs of a CU (tools/microbench/salu_issue.hip: 540 G
// scalar instructions per second for the whole chip, and one scalar instruction among four multiply-adds costs those a third of their rate), so the
// light-sample kernel's 0.78 scalar instructions per vector one were a bound of their own.
// Each comparison is balloted by itself (its own result register) and the masks are combined by scalar instructions: the ballot of a compound
// predicate is compiled as a select and a second comparison.  `undecided` may hold bits of lanes that do not run the test: the caller masks it.
PT_HD void aabb_wave_thick(F4 a, F4 b, const RayPrep& rp, float* entry, uint64_t* hit, uint64_t* undecided) {
    PT_STAT(box_tests);
    float p0 = approx_fma(a.x, rp.r.x, rp.nor.x), q0 = approx_fma(b.x, rp.r.x, rp.nor.x);
    float p1 = approx_fma(a.y, rp.r.y, rp.nor.y), q1 = approx_fma(b.y, rp.r.y, rp.nor.y);
    float p2 = approx_fma(a.z, rp.r.z, rp.nor.z), q2 = approx_fma(b.z, rp.r.z, rp.nor.z);
    float n0 = __builtin_fminf(p0, q0), x0 = __builtin_fmaxf(p0, q0), n1 = __builtin_fminf(p1, q1), x1 = __builtin_fmaxf(p1, q1);
    float n2 = __builtin_fminf(p2, q2), x2 = __builtin_fmaxf(p2, q2);
    float lo = slab_entry(n0, n1, n2), hi = slab_exit(x0, x1, x2);
    float e = approx_fma(PT_SLAB_EPS, lo + pt_abs(hi), rp.base), gap = lo - hi;
    *entry = lo;
    const uint64_t H = PT_WAVE_BALLOT(gap < -e), N = PT_WAVE_BALLOT(!(gap > e));   // (N: not a miss — the negated comparison is one instruction)
    *hit = H; *undecided = N & ~H;
}
PT_HD void aabb_wave_flat(F4 a, F4 b, const RayPrep& rp, float* entry, uint64_t* hit, uint64_t* undecided) {
    PT_STAT(box_tests);
    float p0 = approx_fma(a.x, rp.r.x, rp.nor.x), q0 = approx_fma(b.x, rp.r.x, rp.nor.x);
    float p1 = approx_fma(a.y, rp.r.y, rp.nor.y), q1 = approx_fma(b.y, rp.r.y, rp.nor.y);
    float p2 = approx_fma(a.z, rp.r.z, rp.nor.z), q2 = approx_fma(b.z, rp.r.z, rp.nor.z);
    float n0 = __builtin_fminf(p0, q0), x0 = __builtin_fmaxf(p0, q0), n1 = __builtin_fminf(p1, q1), x1 = __builtin_fmaxf(p1, q1);
    float n2 = __builtin_fminf(p2, q2), x2 = __builtin_fmaxf(p2, q2);
    float m0 = __builtin_fmaxf(__builtin_fmaxf(n1, n2), 0.0f), m1 = __builtin_fmaxf(__builtin_fmaxf(n0, n2), 0.0f), m2 = __builtin_fmaxf(__builtin_fmaxf(n0, n1), 0.0f);
    float e0 = approx_fma(PT_SLAB_EPS, m0 + pt_abs(x0), rp.base), e1 = approx_fma(PT_SLAB_EPS, m1 + pt_abs(x1), rp.base), e2 = approx_fma(PT_SLAB_EPS, m2 + pt_abs(x2), rp.base);
    *entry = __builtin_fmaxf(m0, n0);
    const uint64_t N = PT_WAVE_BALLOT(!(m0 > x0 + e0)) & PT_WAVE_BALLOT(!(m1 > x1 + e1)) & PT_WAVE_BALLOT(!(m2 > x2 + e2));
    const uint64_t H = PT_WAVE_BALLOT(m0 < x0 - e0) & PT_WAVE_BALLOT(m1 < x1 - e1) & PT_WAVE_BALLOT(m2 < x2 - e2) & N;
    *hit = H; *undecided = N & ~H;
}
// A box that is flat along exactly one axis K (every axis-aligned wall): both planes of that axis are the same plane, reached at t_K,
// and AABB::hit's decision — max(entries, 0) <= min(exits) on the quotients it computes — is t_K >= max(n_i, n_l, 0) and
// t_K <= min(x_i, x_l) for the other two axes i, l (n <= x holds per axis by construction, n_K = x_K = t_K exactly: the same division
// twice).  Five planes instead of six and two comparisons instead of three pairs; same margin rule as above.
// The form the host chose for a box (pt_scene_host.cpp flat_code): 0 thick, 1..3 flat along one axis, 4 flat along several (aabb_classify_wave below).
template <int K>
PT_HD void aabb_wave_flat1(F4 a, F4 b, const RayPrep& rp, float* entry, uint64_t* hit, uint64_t* undecided) {
    PT_STAT(box_tests);
    const float ak = K == 0 ? a.x : (K == 1 ? a.y : a.z), rk = K == 0 ? rp.r.x : (K == 1 ? rp.r.y : rp.r.z), nk = K == 0 ? rp.nor.x : (K == 1 ? rp.nor.y : rp.nor.z);
    const float ai = K == 0 ? a.y : a.x, bi = K == 0 ? b.y : b.x, ri = K == 0 ? rp.r.y : rp.r.x, ni_ = K == 0 ? rp.nor.y : rp.nor.x;
    const float al = K == 2 ? a.y : a.z, bl = K == 2 ? b.y : b.z, rl = K == 2 ? rp.r.y : rp.r.z, nl_ = K == 2 ? rp.nor.y : rp.nor.z;
    const float tk = approx_fma(ak, rk, nk);
    const float pi = approx_fma(ai, ri, ni_), qi = approx_fma(bi, ri, ni_), pl = approx_fma(al, rl, nl_), ql = approx_fma(bl, rl, nl_);
    const float n_i = __builtin_fminf(pi, qi), x_i = __builtin_fmaxf(pi, qi), n_l = __builtin_fminf(pl, ql), x_l = __builtin_fmaxf(pl, ql);
    const float lo = slab_entry(n_i, n_l, n_l), hi = __builtin_fminf(x_i, x_l);
    const float e = approx_fma(PT_SLAB_EPS, (lo + pt_abs(hi)) + pt_abs(tk), rp.base);
    const float g1 = lo - tk, g2 = tk - hi;
    *entry = tk;
    const uint64_t H = PT_WAVE_BALLOT(g1 < -e) & PT_WAVE_BALLOT(g2 < -e), N = PT_WAVE_BALLOT(!(g1 > e)) & PT_WAVE_BALLOT(!(g2 > e));
    *hit = H; *undecided = N & ~H;
}
template <int CODE>
PT_HD void aabb_classify_wave(F4 a, F4 b, const RayPrep& rp, float* entry, uint64_t* hit, uint64_t* undecided) {
    if (CODE == 0) aabb_wave_thick(a, b, rp, entry, hit, undecided);
    else if (CODE == 1) aabb_wave_flat1<0>(a, b, rp, entry, hit, undecided);
    else if (CODE == 2) aabb_wave_flat1<1>(a, b, rp, entry, hit, undecided);
    else if (CODE == 3) aabb_wave_flat1<2>(a, b, rp, entry, hit, undecided);
    else aabb_wave_flat(a, b, rp, entry, hit, undecided);
}
PT_HD void aabb_classify_wave_by(uint32_t code, F4 a, F4 b, const RayPrep& rp, float* entry, uint64_t* hit, uint64_t* undecided) {   // `code` wave-uniform
    switch (code) {
        case 0: aabb_classify_wave<0>(a, b, rp, entry, hit, undecided); break;
        case 1: aabb_classify_wave<1>(a, b, rp, entry, hit, undecided); break;
        case 2: aabb_classify_wave<2>(a, b, rp, entry, hit, undecided); break;
        case 3: aabb_classify_wave<3>(a, b, rp, entry, hit, undecided); break;
        default: aabb_classify_wave<4>(a, b, rp, entry, hit, undecided); break;
    }
}
// (the same as one three-way value, for the per-lane loops — BVH walk steps, mesh sweep — whose compiled form is better with it)
PT_HD int aabb_classify(F4 a, F4 b, const RayPrep& rp, bool flat, float* entry, float* exit = nullptr) {   // (`exit`: the distance at which the ray leaves the box, for callers that rank boxes)
    PT_STAT(box_tests);
    float p0 = approx_fma(a.x, rp.r.x, rp.nor.x), q0 = approx_fma(b.x, rp.r.x, rp.nor.x);
    float p1 = approx_fma(a.y, rp.r.y, rp.nor.y), q1 = approx_fma(b.y, rp.r.y, rp.nor.y);
    float p2 = approx_fma(a.z, rp.r.z, rp.nor.z), q2 = approx_fma(b.z, rp.r.z, rp.nor.z);
    float n0 = __builtin_fminf(p0, q0), x0 = __builtin_fmaxf(p0, q0), n1 = __builtin_fminf(p1, q1), x1 = __builtin_fmaxf(p1, q1);
    float n2 = __builtin_fminf(p2, q2), x2 = __builtin_fmaxf(p2, q2);
    if (!flat) {
        float lo = slab_entry(n0, n1, n2), hi = slab_exit(x0, x1, x2);
        float e = approx_fma(PT_SLAB_EPS, lo + pt_abs(hi), rp.base), gap = lo - hi;
        *entry = lo;
        if (exit != nullptr) *exit = hi;
        return gap > e ? 0 : (gap < -e ? 1 : 2);
    }
    if (exit != nullptr) *exit = slab_exit(x0, x1, x2);
    float m0 = __builtin_fmaxf(__builtin_fmaxf(n1, n2), 0.0f), m1 = __builtin_fmaxf(__builtin_fmaxf(n0, n2), 0.0f), m2 = __builtin_fmaxf(__builtin_fmaxf(n0, n1), 0.0f);
    float e0 = approx_fma(PT_SLAB_EPS, m0 + pt_abs(x0), rp.base), e1 = approx_fma(PT_SLAB_EPS, m1 + pt_abs(x1), rp.base), e2 = approx_fma(PT_SLAB_EPS, m2 + pt_abs(x2), rp.base);
    *entry = __builtin_fmaxf(m0, n0);
    if (m0 > x0 + e0 || m1 > x1 + e1 || m2 > x2 + e2) return 0;
    return (m0 < x0 - e0 && m1 < x1 - e1 && m2 < x2 - e2) ? 1 : 2;
}


// The box test of a BVH walk step: the three-way classification when the ray allows it (`quick`: rp.fast and no zero direction
// component; a node with thickness takes the cheap form, a flat one the per-axis form — lanes of a wave stand on different nodes
// here, so two forms, not five), the per-axis filtered test otherwise; the exact test settles what is left.
PT_HD bool aabb_hit_node(F4 a, F4 b, const RayPrep& rp, bool quick, float* entry) {
    if (!quick) return aabb_hit(a, b, rp, entry);
    const int c = aabb_classify(a, b, rp, (pt_f2u(a.w) & PT_NODE_FLAT) != 0u, entry);
    if (c != 2) return c == 1;
    PT_STAT(box_exact);
    return aabb_hit_exact(a, b, rp.o, rp.d, entry);
}
// The box test of a walk step as data flow (the lanes of a wave stand on different nodes): the thick form for every lane, the per-axis form on top of it
// in the waves where some lane stands on a flat node, the exact test in the waves where some lane's decision is too close to call or whose ray the filter
// does not take — three wave-uniform branches instead of a nest of divergent ones (the scalar unit: aabb_classify_wave).  Decisions are the exact test's.
PT_HD bool walk_box(F4 a, F4 b, const RayPrep& rp, bool quick, float* entry) {
    PT_STAT(box_tests);
    const bool flat = ((pt_f2u(a.w) & PT_NODE_FLAT) != 0u) & quick;
    const float p0 = approx_fma(a.x, rp.r.x, rp.nor.x), q0 = approx_fma(b.x, rp.r.x, rp.nor.x);
    const float p1 = approx_fma(a.y, rp.r.y, rp.nor.y), q1 = approx_fma(b.y, rp.r.y, rp.nor.y);
    const float p2 = approx_fma(a.z, rp.r.z, rp.nor.z), q2 = approx_fma(b.z, rp.r.z, rp.nor.z);
    const float n0 = __builtin_fminf(p0, q0), x0 = __builtin_fmaxf(p0, q0), n1 = __builtin_fminf(p1, q1), x1 = __builtin_fmaxf(p1, q1);
    const float n2 = __builtin_fminf(p2, q2), x2 = __builtin_fmaxf(p2, q2);
    const float lo = slab_entry(n0, n1, n2), hi = slab_exit(x0, x1, x2);
    const float e = approx_fma(PT_SLAB_EPS, lo + pt_abs(hi), rp.base), gap = lo - hi;
    float en = lo;
    bool hit = gap < -e, und = !(gap > e) & !(gap < -e);
    if (PT_WAVE_ANY(flat)) {
        const float m0 = __builtin_fmaxf(__builtin_fmaxf(n1, n2), 0.0f), m1 = __builtin_fmaxf(__builtin_fmaxf(n0, n2), 0.0f), m2 = __builtin_fmaxf(__builtin_fmaxf(n0, n1), 0.0f);
        const float e0 = approx_fma(PT_SLAB_EPS, m0 + pt_abs(x0), rp.base), e1 = approx_fma(PT_SLAB_EPS, m1 + pt_abs(x1), rp.base), e2 = approx_fma(PT_SLAB_EPS, m2 + pt_abs(x2), rp.base);
        const bool miss = (m0 > x0 + e0) | (m1 > x1 + e1) | (m2 > x2 + e2);
        const bool hitf = !miss & (m0 < x0 - e0) & (m1 < x1 - e1) & (m2 < x2 - e2);
        hit = flat ? hitf : hit; und = flat ? !miss & !hitf : und; en = flat ? __builtin_fmaxf(m0, n0) : en;
    }
    hit = hit & quick; und = und | !quick;
    if (PT_WAVE_ANY(und)) {
        PT_KEEP_BRANCH();
        if (und) { PT_STAT(box_exact); hit = aabb_hit_exact(a, b, rp.o, rp.d, &en); }
    }
    *entry = en;
    return hit;
}

// MeshTriangleRef::hit (src/geometry/mesh.rs:67-198), split: the per-ray part (axis permutation and shear constants,
// mesh.rs:79-99) is computed once per mesh visit, the interval test per triangle, the HitRecord only for the triangle
// that survives as closest.
struct TriHit { float t, b0, b1, b2; };
PT_HD F3 tri_shuffle(F3 v, uint32_t m) {
    if (m == 0) return f3(v.y, v.z, v.x);
    if (m == 1) return f3(v.z, v.x, v.y);
    return v;
}
struct TriRay { F3 o; uint32_t kz; float sx, sy, sz; F3 os; /* o, permuted like the direction */ };
PT_HD TriRay tri_ray_prepare(F3 o, F3 dir) {
    TriRay r; r.o = o;
    float ax = pt_abs(dir.x), ay = pt_abs(dir.y), az = pt_abs(dir.z);
    float mx = __builtin_fmaxf(__builtin_fmaxf(ax, ay), __builtin_fmaxf(az, 0.0f));
    uint32_t kz = 0;
    if (ax >= mx) kz = 0;
    if (ay >= mx) kz = 1;
    if (az >= mx) kz = 2;
    if (0.0f >= mx) kz = 3;
    F3 d = tri_shuffle(dir, kz);
    r.kz = kz; r.sx = -d.x / d.z; r.sy = -d.y / d.z; r.sz = 1.0f / d.z;
    r.os = tri_shuffle(o, kz);
    return r;
}
// the test proper, on vertices already translated to the ray origin and permuted (mesh.rs:101-198), in two steps: everything that
// does not depend on the interval (edge functions with the f64 fallback, sign test, determinant, scaled distance) ...
// The rejections are written as data flow — one predicate, combined with `&` and `|`, no early return: every divergent `if` costs three scalar instructions
// (save exec, branch, restore) and a predicate that leaves it three more, and the scalar unit is a bound of these kernels (aabb_classify_wave).  A rejected
// lane computes a few more products than it needs; it would have idled through them.
struct TriEdges { float e0, e1, e2, det, ts; };
PT_HD bool triangle_edges(F3 p0t, F3 p1t, F3 p2t, const TriRay& r, TriEdges* g) {
    PT_STAT(tri_tests);
    float sx = r.sx, sy = r.sy, sz = r.sz;
    p0t.x += sx * p0t.z; p1t.x += sx * p1t.z; p2t.x += sx * p2t.z;
    p0t.y += sy * p0t.z; p1t.y += sy * p1t.z; p2t.y += sy * p2t.z;
    float e0 = p1t.x * p2t.y - p1t.y * p2t.x;
    float e1 = p2t.x * p0t.y - p2t.y * p0t.x;
    float e2 = p0t.x * p1t.y - p0t.y * p1t.x;
    const bool zero_edge = (e0 == 0.0f) | (e1 == 0.0f) | (e2 == 0.0f);
    if (PT_WAVE_ANY(zero_edge)) {   // (rare: a wave-uniform branch around the lanes that need the f64 edge functions)
        PT_KEEP_BRANCH();
        if (zero_edge) {
            double a = (double)p2t.x * (double)p1t.y, b = (double)p2t.y * (double)p1t.x;
            e0 = (float)(b - a);
            a = (double)p0t.x * (double)p2t.y; b = (double)p0t.y * (double)p2t.x;
            e1 = (float)(b - a);
            a = (double)p1t.x * (double)p0t.y; b = (double)p1t.y * (double)p0t.x;
            e2 = (float)(b - a);
        }
    }
    // some edge function negative and some positive: the minimum and the maximum of the three (a NaN is ignored by both, as by the six comparisons)
    const bool mixed = (slab_exit(e0, e1, e2) < 0.0f) & (pt_max3(e0, e1, e2) > 0.0f);
    float det = e0 + e1 + e2;
    p0t.z *= sz; p1t.z *= sz; p2t.z *= sz;
    g->e0 = e0; g->e1 = e1; g->e2 = e2; g->det = det;
    g->ts = e0 * p0t.z + e1 * p1t.z + e2 * p2t.z;
    return !mixed & (det != 0.0f);
}
// ... and the interval test in its scaled form (mesh.rs:150-158): true when (ts, det) lies outside (t0, t1]
PT_HD bool triangle_outside(float ts, float det, float t0, float t1) {
    const float a = t0 * det, b = t1 * det;
    return ((det < 0.0f) & ((ts >= a) | (ts < b))) | ((det > 0.0f) & ((ts <= a) | (ts > b)));
}
PT_HD bool triangle_test_core(F3 p0t, F3 p1t, F3 p2t, const TriRay& r, float t0, float t1, TriHit* out) {
    TriEdges g;
    const bool inside = triangle_edges(p0t, p1t, p2t, r, &g);
    if (!(inside & !triangle_outside(g.ts, g.det, t0, t1))) return false;
    float inv_det = 1.0f / g.det;
    out->b0 = g.e0 * inv_det; out->b1 = g.e1 * inv_det; out->b2 = g.e2 * inv_det;
    out->t = g.ts * inv_det;
    return true;
}
PT_HD bool triangle_test(F3 p0, F3 p1, F3 p2, const TriRay& r, float t0, float t1, TriHit* out) {
    return triangle_test_core(tri_shuffle(sub(p0, r.o), r.kz), tri_shuffle(sub(p1, r.o), r.kz), tri_shuffle(sub(p2, r.o), r.kz), r, t0, t1, out);
}
// Vertices stored already permuted for the ray's dominant axis (the sweep table's triangles are kept in all three
// permutations, pt_blob.h): permuting commutes with the subtraction, so the 18 selects per test go away — same bits.
PT_HD bool triangle_test_permuted(F3 p0s, F3 p1s, F3 p2s, const TriRay& r, float t0, float t1, TriHit* out) {
    return triangle_test_core(sub(p0s, r.os), sub(p1s, r.os), sub(p2s, r.os), r, t0, t1, out);
}

PT_HD F3 rect_shuffle(F3 v, uint32_t axis) {
    if (axis == PT_AXIS_X) return f3(v.z, v.y, v.x);
    if (axis == PT_AXIS_Y) return f3(v.x, v.z, v.y);
    return v;
}
PT_HD F3 axis_vec(uint32_t axis) { return axis == PT_AXIS_X ? f3(1, 0, 0) : (axis == PT_AXIS_Y ? f3(0, 1, 0) : f3(0, 0, 1)); }

// Aggregate::hit for rect / sphere / disk (src/geometry/rect.rs:69-112, sphere.rs:34-87, disk.rs:31-62); tmax = inf on this path.
PT_HD bool analytic_hit(const SceneView& s, uint32_t inst, uint32_t kind, F3 o, F3 d, float t1, Hit* out) {
    uint32_t flags = bu(s, inst + PT_INST_FLAGS);
    bool two_sided = (flags & 2u) != 0;
    F3 origin = bf3(s, inst + PT_INST_ORIGIN);
    const uint32_t mat0 = PT_MATERIAL_ID(PT_TAG_MATERIAL, 0);
    if (kind == PT_SHAPE_RECT) {
        uint32_t axis = (flags >> 2) & 3u;
        float s0 = bf(s, inst + PT_INST_SIZE), s1 = bf(s, inst + PT_INST_SIZE + 1);
        F3 to = rect_shuffle(sub(o, origin), axis), td = rect_shuffle(d, axis);
        // one predicate, no early return (triangle_edges); a ray in the plane divides by zero into an inf or a NaN that the first term rejects
        float t = (-to.z) / td.z;
        float xh = to.x + t * td.x, yh = to.y + t * td.y;
        float hx = s0 / 2.0f, hy = s1 / 2.0f;
        const bool out_of_range = (td.z == 0.0f) | (t <= 0.0f) | (t > t1) | (t >= PT_INF);
        const bool off_rect = (xh < -hx) | (xh > hx) | (yh < -hy) | (yh > hy);
        if (out_of_range | off_rect) return false;
        F3 n = axis_vec(axis);
        if (two_sided && dot(d, n) > 0.0f) n = neg(n);
        out->t = t; out->p = add(o, mul(d, t)); out->u = (xh + hx) / s0; out->v = (yh + hy) / s1;
        // HitRecord::new normalizes the normal (hittable.rs:30-39); n is +-e_axis: norm = sqrt(1) = 1 and x / 1 = x, bit for bit
        out->n = n; out->material = mat0; out->valid = true;
        return true;
    }
    if (kind == PT_SHAPE_SPHERE) {
        float radius = bf(s, inst + PT_INST_RADIUS);
        F3 oc = sub(o, origin);
        float a = dot(d, d), b = dot(oc, d), c = dot(oc, oc) - radius * radius;
        float disc = b * b - a * c;
        if (!(disc > 0.0f)) return false;
        float ds = pt_sqrt(disc);
        float t = (-b - ds) / a;
        if (!(t < t1 && t > 0.0f && t < PT_INF)) {
            t = (-b + ds) / a;
            if (!(t < t1 && t > 0.0f && t < PT_INF)) return false;
        }
        F3 p = add(o, mul(d, t));
        out->t = t; out->p = p; out->u = 0.0f; out->v = 0.0f;
        out->n = normalize(divs(sub(p, origin), radius)); out->material = mat0; out->valid = true;
        return true;
    }
    // disk
    float radius = bf(s, inst + PT_INST_RADIUS);
    F3 to = sub(o, origin);
    float t = (-to.z) / d.z;
    float xh = to.x + t * d.x, yh = to.y + t * d.y;
    if ((d.z == 0.0f) | (t <= 0.0f) | (t > t1) | (t >= PT_INF) | (xh * xh + yh * yh > radius * radius)) return false;
    F3 n = f3(0, 0, 1);
    if (dot(d, n) > 0.0f && two_sided) n = neg(n);
    out->t = t; out->p = add(o, mul(d, t)); out->u = 0.0f; out->v = 0.0f;
    out->n = n; out->material = mat0; out->valid = true;  // (0, 0, +-1): normalizing it changes no bit
    return true;
}

// World::hit(r, 0, inf): Accelerator::hit (src/accelerator/mod.rs:106-176) + FlatBVH::traverse (lbvh.rs:172-213) +
// Instance::hit (instance.rs:75-133) + Mesh::hit (mesh.rs:314-360), as ONE loop.
//
// The reference nests two walks (instances, then the triangles of a mesh instance).  Nested loops are poison for a
// wave64: lanes reach mesh leaves at different outer iterations, so every inner walk runs with a handful of lanes
// (measured: 6400 VALU instructions per wave-ray for a lane average of 15 box tests).  Here a lane is a small state
// machine — (level, node index, current ray) — and every loop iteration performs exactly one box test, whether the
// lane is at the top level or inside a mesh, so the box-test instructions are shared by all lanes.  Each lane still
// visits its nodes, instances and triangles in exactly the reference's order (ties are broken by that order: rect /
// disk / triangle accept t <= closest, sphere t < closest), and the HitRecord is built once, after the walk, from
// (instance, triangle, barycentrics) or by re-running the analytic test — same arithmetic, same bits.
PT_HD void instance_local_ray(const SceneView& s, uint32_t inst, F3 o, F3 d, F3* lo, F3* ld) {
    if (instance_is_transformed(s, inst)) { *lo = xf_point(s, inst + PT_INST_REVERSE, o); *ld = xf_vec(s, inst + PT_INST_REVERSE, d); }
    else { *lo = o; *ld = d; }
}
// HitRecord of the winning primitive (Instance::hit, instance.rs:89-131; mesh.rs:160-197): `triw` is the word offset of the
// winning triangle, or 0 for an analytic instance, whose test is re-run (the accepted root does not depend on the upper
// bound it was tested against).
PT_HD void hit_record(const SceneView& s, F3 o, F3 d, uint32_t best_inst, uint32_t triw, const TriHit& bh, Hit* out) {
    uint32_t inst = bu(s, PT_HDR_INSTANCE_OFF) + best_inst * PT_INST_WORDS;
    F3 lo, ld;
    instance_local_ray(s, inst, o, d, &lo, &ld);
    Hit h;
    uint32_t in_safe = 0u;   // PT_HIT_IN_SAFE and the outward threshold of the face (pt_blob.h PT_TRI_FLAGS), handed to the vertex code in the instance word
    float area = 0.0f;       // the face's A_f (the spare word of its normal record, pt_blob.h PT_HDR_LIGHT_FACE_OFF): 0 unless it is an emissive face
    if (triw != 0u) {
        uint32_t mesh = bu(s, inst + PT_INST_MESH);
        uint32_t normal_off = bu(s, mesh + PT_MESH_NORMAL_OFF);
        F4 q0 = mf4(s, triw), q1 = mf4(s, triw + 4), q2 = mf4(s, triw + 8);
        if (scene_has_certificates(s)) {   // (a scalar branch.  The face's flag word, pt_blob.h PT_TRI_FLAGS: bit 0 the inward claim for the whole face, bit 1 for its inside,
            PT_KEEP_BRANCH_NOFENCE();      // away from the edges by PT_TRI_INNER_BARY; bits 2.. the outward threshold, handed on as it is)
            const uint32_t tf = pt_f2u(q2.w);
            const bool inner = __builtin_fminf(__builtin_fminf(bh.b0, bh.b1), bh.b2) >= PT_TRI_INNER_BARY;
            in_safe = ((tf | (inner ? tf >> 1 : 0u)) & 1u) << 31 | ((tf >> PT_TRI_OUT_SHIFT) & 0x7fffu) << PT_HIT_OUT_SHIFT;
        }
        F3 p0 = f3(q0.x, q0.y, q0.z), p1 = f3(q1.x, q1.y, q1.z), p2 = f3(q2.x, q2.y, q2.z);
        if (normal_off != 0) {
            uint32_t nn = normal_off + (triw - bu(s, mesh + PT_MESH_TRI_OFF));
            F4 m0 = mf4(s, nn), m1 = mf4(s, nn + 4), m2 = mf4(s, nn + 8);
            F3 n = add(add(mul(f3(m0.x, m0.y, m0.z), bh.b0), mul(f3(m1.x, m1.y, m1.z), bh.b1)), mul(f3(m2.x, m2.y, m2.z), bh.b2));
            h.n = normalize(n);
            area = m0.w;
        } else {
            // the face normal, normalize(normalize(cross(p0 - p2, p1 - p2))), as the host computed it with these same functions (pt_scene_host.cpp)
            const F4 fn = mf4(s, pt_f2u(q1.w));
            h.n = f3(fn.x, fn.y, fn.z);
            area = fn.w;
        }
        h.t = bh.t;
        h.p = add(add(mul(p0, bh.b0), mul(p1, bh.b1)), mul(p2, bh.b2));
        h.u = 0.0f; h.v = 0.0f;
        h.material = pt_f2u(q0.w);
    } else {
        analytic_hit(s, inst, bu(s, inst + PT_INST_KIND), lo, ld, PT_INF, &h);
    }
    if (instance_is_transformed(s, inst)) {
        h.n = normalize(xf_vec_transposed(s, inst + PT_INST_REVERSE, h.n));
        h.p = xf_point(s, inst + PT_INST_FORWARD, h.p);
    }
    h.instance = best_inst | in_safe;
    uint32_t m = bu(s, inst + PT_INST_MATERIAL);
    if (m != PT_MATERIAL_NONE) h.material = m;
    // A light-tagged hit on a mesh face carries the face's area in u (a mesh hit's u is 0, and no light material reads a texture): the BSDF-hit MIS weight at such a
    // vertex needs 1 / A_f (light_psa_pdf), and the hit queue has no word for the face.  Compiled out of every form of a scene without emissive faces.
    if (!(s.lacks & PT_SCENE_NO_MESH_LIGHTS) && triw != 0u && PT_MATERIAL_TAG(h.material) == PT_TAG_LIGHT) h.u = area;
    h.valid = true;
    *out = h;
}

// ---- leaf sweep: World::hit for scenes of at most 64 leaves ------------------------------------------------------------
// The reference's walk tests exactly the leaves whose own box passes AABB::hit (a triangle leaf: its box and its
// instance's box) — ancestor boxes contain them and the slab test is monotone under rounding, so they pass too — in
// pre-order, against the running closest hit.  For a scene this small the tree walk is therefore replaced by
//   1. a sweep over ALL leaf boxes with wave-uniform addresses and no divergence (every lane of the wave executes the
//      same box test on the same box), collecting per lane a 64-bit mask of hit leaves and a mask of undecided ones,
//   2. the exact six-division test for the undecided bits only,
//   3. the primitive tests of the lane's hit leaves in bit order = pre-order.
// Same leaves, same order, same arithmetic as world_hit: same bits.  The tree walk keeps 32 % of the VALU lanes busy
// (profiles/r1c); here step 1, the bulk of the work, keeps all of them busy.
PT_HD uint32_t ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }
// Phases 1 and 2: the mask of leaves whose own box the ray hits (walked mesh instances keep their instance bit).
PT_HD uint64_t sweep_masks(const SceneView& s, F3 o, F3 d, float bound) {
    // (header words made scalars once: the loop's counter and addresses stay in the scalar unit without a read-first-lane per turn)
    const uint32_t flags = PT_UNIFORM(bu(s, PT_HDR_FLAGS)), sweep = PT_UNIFORM(bu(s, PT_HDR_SWEEP_OFF)), count = PT_UNIFORM(bu(s, PT_HDR_SWEEP_COUNT)), bits_off = bu(s, PT_HDR_SWEEP_BITS_OFF);
    const bool exact = (flags & PT_FLAG_EXACT_SLAB) != 0;
    const bool cull_top = (flags & (PT_FLAG_NO_TOP_CULL | PT_FLAG_NO_CULL)) == 0, cull_mesh = (flags & PT_FLAG_NO_CULL) == 0;
    const RayPrep wr = ray_prepare(o, d);
    const bool quick = wr.fast & !exact & (d.x != 0.0f) & (d.y != 0.0f) & (d.z != 0.0f);
    const bool bounded = bound < PT_INF;
    // the masks are built as 32-bit halves
    uint32_t hit_lo = 0, hit_hi = 0, unc_lo = 0, unc_hi = 0;
    PT_STAT_EVENT(0);
    PT_STAT_RAY(o, d);
    // 1 — the sweep.  `bound` culls leaves that start beyond the distance the caller cares about (shadow rays).
    // A test sets a whole mask: the leaf's bit and the bits of the later leaves of the instance with the very same box (same box,
    // same ray, same decision; the host folds them into the mask, pt_blob.h).  Every mask word costs one select-and-or.
    // An undecided box is rare (0.8 % of the rays meet one): its masks are touched only in the waves where some lane has one — a
    // scalar test of the wave mask instead of four vector instructions per box.
    // The decisions are wave masks (aabb_classify_wave): the lanes whose ray the filter takes (`q`) run the test, the others are undecided at every box;
    // on the device every lane computes (a lane outside `q` computes on values the filter's bounds do not cover: its bits are masked, nothing reads them).
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool every_lane = true;
#else
    constexpr bool every_lane = false;   // (the emulation's one lane: the test only where the device's result would be read; PT_STAT counts those)
#endif
    const uint64_t q = PT_WAVE_BALLOT(quick), nq = PT_WAVE_BALLOT(!quick);
    // beyond(entry, bound, base) with the flag folded into the bound: a search that may not cull compares with +inf (never beyond)
    const float bound_top = cull_top ? bound : PT_INF, bound_mesh = cull_mesh ? bound : PT_INF;
    auto mark = [&](uint64_t H, uint64_t U, uint32_t mlo, uint32_t mhi) {
        const bool hl = PT_WAVE_MEMBER(H);
        hit_lo |= hl ? mlo : 0u; hit_hi |= hl ? mhi : 0u;
        if (U != 0ull) { PT_KEEP_BRANCH(); const bool ul = PT_WAVE_MEMBER(U); unc_lo |= ul ? mlo : 0u; unc_hi |= ul ? mhi : 0u; }
    };
    // the instances whose box test is all there is to do (PT_HDR_SWEEP_SIMPLE): one tight loop per form of the test
    uint32_t first_general = 0u;
    {
        uint32_t e = sweep;
        auto simple = [&](auto code, uint32_t n) {
            first_general += n;
            for (; n != 0u; --n, e += PT_SWEEP_INST_WORDS) {
                const F4 h0 = bf4(s, e), a = bf4(s, e + 4), b = bf4(s, e + 8);
                float entry = 0.0f;
                uint64_t ih = 0ull, iu = 0ull;
                if (every_lane || q != 0ull) aabb_classify_wave<decltype(code)::value>(a, b, wr, &entry, &ih, &iu);
                ih &= q; iu = (iu & q) | nq;
                ih &= ~PT_WAVE_BALLOT(beyond(entry, bound_top, wr.base));
                mark(ih, iu, pt_f2u(h0.z), pt_f2u(h0.w));
            }
        };
        const uint32_t sizes = PT_UNIFORM(bu(s, PT_HDR_SWEEP_SIMPLE));
        simple(IntC<0>(), sizes & 0xffu); simple(IntC<1>(), (sizes >> 8) & 0xffu); simple(IntC<2>(), (sizes >> 16) & 0xffu); simple(IntC<3>(), sizes >> 24);
        simple(IntC<4>(), PT_UNIFORM(bu(s, PT_HDR_SWEEP_SIMPLE + 1)));
    }
    for (uint32_t j = first_general; j < count; ++j) {
        const uint32_t e = PT_UNIFORM(sweep + j * PT_SWEEP_INST_WORDS);
        const F4 h0 = bf4(s, e), a = bf4(s, e + 4), b = bf4(s, e + 8);
        const uint32_t kf = PT_UNIFORM(pt_f2u(h0.y));
        float entry = 0.0f;
        uint64_t ih = 0ull, iu = 0ull;
        // (An untransformed mesh instance's box holds every box of its leaves, so its own test decides nothing — but it lets a wave whose
        // rays all miss the instance skip the leaves: without it C2's k_extend takes 2360 us instead of 2283, k_shadow 4648 instead of 4466.)
        if (every_lane || q != 0ull) aabb_classify_wave_by((kf >> 11) & 7u, a, b, wr, &entry, &ih, &iu);
        ih &= q; iu = (iu & q) | nq;   // (a ray the filter cannot take: every box is undecided)
        // (`bound` = inf culls nothing: the comparison is false)
        if ((kf & 0xffu) != PT_SHAPE_SPHERE) ih &= ~PT_WAVE_BALLOT(beyond(entry, bound_top, wr.base));
        mark(ih, iu, pt_f2u(h0.z), pt_f2u(h0.w));
        const uint64_t inside = ih | iu;
        if ((kf & (0xffu | PT_SWEEP_WALKED)) == PT_SHAPE_MESH && (kf >> 24) != 0u && inside != 0ull) {
            const uint32_t tl = PT_UNIFORM(pt_f2u(a.w)), tc = kf >> 24;   // the leaves with a box test of their own
            const uint32_t groups = PT_UNIFORM(pt_f2u(bf4(s, e + 12).x));   // the leaves come grouped by the form of their box test
            // the triangle leaves against the instance's ray: the world ray itself unless the instance is transformed (a branch
            // on a wave-uniform flag, not a copy of the prepared ray: 20 registers moved per mesh instance otherwise)
            auto leaves = [&](const RayPrep& lr, uint64_t lq, uint64_t lnq) {
                const uint64_t qi = lq & inside, nqi = lnq & inside;
                uint32_t t = 0;
                auto group = [&](auto code, uint32_t n) {
                    for (const uint32_t end = t + n; t < end; ++t) {
                        const F4 ta = bf4(s, tl + t * PT_SWEEP_TRI_WORDS), tb = bf4(s, tl + t * PT_SWEEP_TRI_WORDS + 4);
                        uint64_t th = 0ull, tu = 0ull;
                        if (every_lane || qi != 0ull) aabb_classify_wave<decltype(code)::value>(ta, tb, lr, &entry, &th, &tu);
                        th &= qi; tu = (tu & qi) | nqi;
                        th &= ~PT_WAVE_BALLOT(beyond(entry, bound_mesh, lr.base));
                        mark(th, tu, pt_f2u(ta.w), pt_f2u(tb.w));
                    }
                };
                const uint32_t n0 = groups & 0xffu, n1 = (groups >> 8) & 0xffu, n2 = (groups >> 16) & 0xffu, n3 = groups >> 24;
                group(IntC<0>(), n0); group(IntC<1>(), n1); group(IntC<2>(), n2); group(IntC<3>(), n3); group(IntC<4>(), tc - (n0 + n1 + n2 + n3));
            };
            if (sweep_leaf_transformed(s, kf)) {
                F3 lo, ld;
                instance_local_ray(s, pt_f2u(h0.x), o, d, &lo, &ld);
                const RayPrep lr = ray_prepare(lo, ld);
                const bool lquick = lr.fast && !exact && ld.x != 0.0f && ld.y != 0.0f && ld.z != 0.0f;
                leaves(lr, PT_WAVE_BALLOT(lquick), PT_WAVE_BALLOT(!lquick));
            } else leaves(wr, q, nq);
        }
    }
    uint64_t hit = (uint64_t)hit_lo | (uint64_t)hit_hi << 32, unc = (uint64_t)unc_lo | (uint64_t)unc_hi << 32;
    // 2 — settle the undecided boxes, ascending, so that an instance box is settled before its triangles'
    while (unc != 0) {
        const uint32_t k = ctz64(unc);
        unc &= unc - 1;
        const F4 be = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS), bg = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS + 4);
        const uint32_t inst = pt_f2u(be.x), triw = pt_f2u(be.y), box = pt_f2u(be.z), kf = pt_f2u(be.w);
        const uint64_t followers = (uint64_t)pt_f2u(bg.x) | (uint64_t)pt_f2u(bg.y) << 32;  // copies of this decision
        F3 ro = o, rd = d;
        if (triw != 0u) instance_local_ray(s, inst, o, d, &ro, &rd);
        float entry;
        PT_STAT(box_exact);
        bool h = aabb_hit_exact(bf4(s, box), bf4(s, box + 4), ro, rd, &entry);
        if (bounded && h && (triw != 0u ? cull_mesh : cull_top) && (kf & 0xffu) != PT_SHAPE_SPHERE && beyond(entry, bound, 0.0f)) h = false;
        unc &= ~followers;
        if (h) hit |= 1ull << k | followers;
        else if (triw == 0u && (kf & (0xffu | PT_SWEEP_WALKED)) == PT_SHAPE_MESH) {
            const uint32_t tc = pt_f2u(bf4(s, box + 4).w);  // triangle-leaf count rides in the instance entry's max.w
            const uint64_t range = (tc + 1 >= 64 ? ~0ull : ((1ull << (tc + 1)) - 1)) << k;
            hit &= ~range; unc &= ~range;
        }
    }
    hit &= ~((uint64_t)bu(s, PT_HDR_SWEEP_MESH_MASK) | (uint64_t)bu(s, PT_HDR_SWEEP_MESH_MASK + 1) << 32);
    return hit;
}

// When a search may end early: never (closest hit wanted), at the first opaque hit in front of every light (light rays, with
// the nearest light hit as bound), or at any accepted hit (environment rays: only "is anything in the way" matters).
enum { PT_STOP_NONE = 0, PT_STOP_NONLIGHT = 1, PT_STOP_ANY = 2 };

// The running state of phase 3 — it can be parked (a lane that reaches a walked mesh) and resumed later.
struct SweepState { uint64_t hit; float closest; uint32_t best_inst, best_triw; TriHit bh; };
PT_HD void sweep_state_init(SweepState& st, uint64_t hit) {
    st.hit = hit; st.closest = PT_INF; st.best_inst = 0xffffffffu; st.best_triw = 0u; st.bh.t = 0.0f; st.bh.b0 = st.bh.b1 = st.bh.b2 = 0.0f;
}
// One ray — every argument the same in all the lanes of `lanes`, the caller's wave — against all the leaves of a mesh, the lanes side by
// side.  For the rays a walk is worst at: AABB::hit ignores an axis along which the direction is zero (aabb.rs:41-45: its slab becomes
// [0, inf) wherever the origin lies), so a ray parallel to an axis passes every box that overlaps it in the other axes only — an environment
// sample at the pole of the map, (0, 0, 1), passes eight in ten of the monkey's 8375 boxes and tests half its triangles: 8000 dependent steps
// of one lane, 3-6 ms, while a wave lives 0.5 ms on average (tools/wave_timeline.py: they were the last third of C4's k_shadow_parked and
// four fifths of its deep bounces).  Same leaves, same order, same arithmetic as the walk, 64 nodes per step: a leaf is tested iff its own box
// passes (the slab test is monotone: then every ancestor passes; the walk's culling by the closest hit only skips leaves whose triangle
// could not be accepted), its triangle against the unbounded interval, and the acceptances are replayed in node order against the running
// closest hit with the walk's own comparison (triangle_outside split in two, as in the pooled sweep) and its early stops.
PT_HD void mesh_scan(const SceneView& s, uint32_t inst, uint32_t node_off, uint32_t node_count, uint32_t tri_off, const RayPrep& cr, const TriRay& tr, float bound, int stop,
                     unsigned long long lanes, float* closest, uint32_t* best_triw, bool* stopped) {
    const uint32_t width = (uint32_t)__builtin_popcountll(lanes), rank = PT_WAVE_RANK(lanes);
    for (uint32_t base = 0; base < node_count; base += width) {
        const uint32_t k = base + rank;
        float ts = 0.0f, det = 0.0f, t = 0.0f;   // (det == 0: this lane holds no candidate)
        uint32_t triw = 0u;
        if (k < node_count) {
            const F4 a = mf4(s, node_off + k * PT_NODE_WORDS), b = mf4(s, node_off + k * PT_NODE_WORDS + 4);
            const uint32_t shape = pt_f2u(b.w);
            float entry;
            if (shape != PT_NODE_INNER && aabb_hit(a, b, cr, &entry)) {
                triw = tri_off + shape * PT_TRI_WORDS;
                const F4 q0 = mf4(s, triw), q1 = mf4(s, triw + 4), q2 = mf4(s, triw + 8);
                TriEdges g;
                if (triangle_edges(tri_shuffle(sub(f3(q0.x, q0.y, q0.z), tr.o), tr.kz), tri_shuffle(sub(f3(q1.x, q1.y, q1.z), tr.o), tr.kz), tri_shuffle(sub(f3(q2.x, q2.y, q2.z), tr.o), tr.kz), tr, &g)
                    && !triangle_outside(g.ts, g.det, 0.0f, PT_INF)) { ts = g.ts; det = g.det; t = g.ts * (1.0f / g.det); }
            }
        }
        unsigned long long m = PT_WAVE_BALLOT(det != 0.0f);
        while (m != 0ull) {
            const uint32_t j = ctz64(m);
            m &= m - 1ull;
            const float tsj = pt_u2f(PT_WAVE_READ(pt_f2u(ts), j)), detj = pt_u2f(PT_WAVE_READ(pt_f2u(det), j));
            if (detj < 0.0f ? tsj < *closest * detj : tsj > *closest * detj) continue;   // (beyond the closest hit so far: triangle_outside's second half)
            const float tj = pt_u2f(PT_WAVE_READ(pt_f2u(t), j));
            if (tj > bound) continue;   // (behind the light that bounds this search: the walk culls such leaves by min(closest, bound) where it can; the answer — is the closest hit a light — is the same either way, round-3 advisor)
            *closest = tj;
            *best_triw = PT_WAVE_READ(triw, j);
            if (stop == PT_STOP_ANY) { *stopped = true; return; }
            if (stop == PT_STOP_NONLIGHT && *closest < bound) {
                const uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                if (PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : mu(s, *best_triw + 3u)) != PT_TAG_LIGHT) { *stopped = true; return; }
            }
        }
    }
}

#if defined(PT_TIMELINE_RAYS)
// (measurement build, tools/wave_timeline.py: the rays whose walk took more than 1500 box tests)
static __device__ float g_tl_rays[1 + 4096 * 12];
#endif
#if defined(PT_TIMELINE_RAYS) && defined(__HIP_DEVICE_COMPILE__)
#define PT_TL_STEP() (++tl_steps)
#define PT_TL_DONE() do { if (tl_steps > 1500u) { const uint32_t e = atomicAdd(reinterpret_cast<uint32_t*>(g_tl_rays), 1u); if (e < 4096u) { float* r = g_tl_rays + 1 + e * 12; \
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; r[6] = bound; r[7] = (float)stop; r[8] = (float)tl_steps; r[9] = lo.x; r[10] = ld.x; r[11] = st.closest; } } } while (0)
#else
#define PT_TL_STEP()
#define PT_TL_DONE()
#endif
// Mesh::hit (src/geometry/mesh.rs:314-360) for one instance, against the running closest hit: the mesh half of
// world_hit_walk on its own (same while-while loop, same filtered box test, same culling).
//
// `policy` (the parked kernels, whose waves are 64 walks; pt_tuning::walk_evict_below | walk_search_below << 8; 0 = the plain loop): a walk's length
// varies by an order of magnitude between the rays of a wave, and so does the number of boxes between one leaf and the next.
//  * Eviction (low byte E, needs `cursor`): after a triangle test, when fewer than E lanes of the wave are still walking, those lanes leave the walk
//    with the node they would visit next in `*cursor` (returns true); the caller parks them again and they go on — from that node, with the closest
//    hit they carry — in a later wave of 64, next to rays that are as far from done as they are.  `*cursor` on entry: where to go on (0 = a walk
//    that has not begun).
//  * Short searches (second byte X): the inner loop — every lane steps from box to box until it holds a leaf — ends once fewer than X lanes are
//    still searching while others hold one: those test their triangles and search on, instead of waiting for the wave's longest search.
//  * Axis rays (PT_WALK_SCAN_AXIS): a ray with a zero direction component is not walked but scanned by the whole wave (mesh_scan).
// A ray's own sequence of tests is untouched by the first two; the third tests the same leaves side by side and replays their order.
#define PT_WALK_SCAN_AXIS 0x10000u
#ifndef PT_SWEEP_FIFO
#define PT_SWEEP_FIFO 1
#endif
#ifndef PT_SWEEP_FIFO_ROUND
#define PT_SWEEP_FIFO_ROUND 32u   /* a round of triangle tests when at least this many lanes hold a leaf (the emulation's lane: never, until its queue fills) */
#endif
// `alive` (the parked kernels' last, partly filled drains): a lane without a ray of its own comes along — with the instance of one that has — to
// take its share of the scans, and leaves before the walk.
// SPEC (round 4): speculation — while any lane of the wave still searches for its first leaf, a lane that holds one searches on for its NEXT one (`pending2`)
// instead of idling; the wave runs its triangle pass when nobody lacks a first leaf.  A lane's leaves keep their order; the box tests of the second search see the
// closest hit from before the first leaf's triangle test, which only lets through boxes whose triangle cannot be accepted (as in the sweep's FIFO).  A lane evicted
// while it holds an untested leaf leaves with that leaf's own node in the cursor: the box is tested again on resume.
// GROUPS (round 5: the round-4 verdict's "entered-group loop without eviction"): in the grouped sweep a lane's ray enters 5.7 groups on average and a wave waits for the lane with
// the most — lane utilisation 0.38.  Once fewer lanes than `(policy >> 17) & 0x7f` still have a group to do, those drain their triangle queues and LEAVE: cursor = PT_GROUPS_EVICTED,
// `*aux` = the mask of their groups still to do (the caller parks both: two words an entry of a path segment has to spare); a later wave of 64 such rays goes straight to its groups.
#define PT_GROUPS_EVICTED 0xfffffffeu
template <bool SPEC = false>
// `inside` (round 6): the ray is KNOWN to start inside this instance, a certified closed convex body (a path segment that left an inward-safe face inward: pt_blob.h
// PT_INST_CONVEX_IN, the mark in its record's slot word).  The ray's line crosses such a body's surface twice, once behind the origin and once in front: only the
// triangle in front can be accepted — so once a triangle is accepted WELL INSIDE itself (every barycentric coordinate >= PT_INSIDE_BARY: the ray passes no edge or vertex of
// the accepted triangle within the reach of rounding, where a neighbour might be accepted too and, later in the order, win a tie), no later leaf of this mesh can be:
// the grouped and plain sweeps and the while-while walk of this mesh end there for this lane.
#define PT_INSIDE_BARY 1e-3f
#ifndef PT_FIRST_RANK
#define PT_FIRST_RANK 0
#endif
#ifndef PT_INSIDE_FIRST_GROUP
#define PT_INSIDE_FIRST_GROUP 0   /* 1: the grouped sweep tries the group an inside ray leaves last first (below; round 6, EXPERIMENT) */
#endif
PT_HD bool mesh_walk(const SceneView& s, uint32_t inst, uint32_t inst_id, F3 o, F3 d, float bound, int stop, SweepState& st,
                     uint32_t* cursor = nullptr, uint32_t policy = 0u, bool alive = true, uint64_t* aux = nullptr, bool inside = false) {
    const uint32_t NONE = 0xffffffffu;
    const uint32_t flags = bu(s, PT_HDR_FLAGS);
    const bool cull = (flags & PT_FLAG_NO_CULL) == 0;
    F3 lo, ld;
    instance_local_ray(s, inst, o, d, &lo, &ld);
    const bool regroup = cursor != nullptr && *cursor == PT_GROUPS_EVICTED;   // (evicted from the grouped sweep's group loop: its groups still to do came along in *aux)
    const uint32_t begin_at = (cursor != nullptr && !regroup) ? *cursor : 0u;   // (a ray that was evicted from a walk goes on walking — and so does its whole wave)
    if (policy & PT_WALK_SCAN_AXIS) {
        // rays parallel to an axis of the mesh: one after the other, the whole wave on each (mesh_scan).  Before this lane's own constants
        // are made: the scan works on the broadcast ray's, and the two sets need not be held at once.
        const bool axis = alive && begin_at == 0u && (ld.x == 0.0f || ld.y == 0.0f || ld.z == 0.0f);
        unsigned long long am = PT_WAVE_BALLOT(axis);
        if (am != 0ull) {
            PT_KEEP_BRANCH();
            const unsigned long long lanes = PT_WAVE_BALLOT(true);
            const uint32_t me = PT_WAVE_RANK(~0ull);
            while (am != 0ull) {
                const uint32_t L = ctz64(am);
                am &= am - 1ull;
                auto rd = [&](float x) { return pt_u2f(PT_WAVE_READ(pt_f2u(x), L)); };
                const F3 ulo = f3(rd(lo.x), rd(lo.y), rd(lo.z)), uld = f3(rd(ld.x), rd(ld.y), rd(ld.z));
                RayPrep ucr = ray_prepare(ulo, uld);
                if (flags & PT_FLAG_EXACT_SLAB) ucr.fast = false;
                const TriRay utr = tri_ray_prepare(ulo, uld);
                const uint32_t uinst = PT_WAVE_READ(inst, L), umesh = bu(s, uinst + PT_INST_MESH);
                float closest = rd(st.closest);
                uint32_t best = 0xffffffffu;
                bool stopped = false;
                mesh_scan(s, uinst, bu(s, umesh + PT_MESH_NODE_OFF), bu(s, umesh + PT_MESH_NODE_COUNT), bu(s, umesh + PT_MESH_TRI_OFF), ucr, utr, rd(bound),
                          (int)PT_WAVE_READ((uint32_t)stop, L), lanes, &closest, &best, &stopped);
                if (me == L && best != 0xffffffffu) {
                    // the winner's record: its test again (the numbers do not depend on the interval)
                    const F4 q0 = mf4(s, best), q1 = mf4(s, best + 4), q2 = mf4(s, best + 8);
                    TriHit th;
                    triangle_test(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), utr, 0.0f, PT_INF, &th);
                    st.closest = th.t; st.best_inst = inst_id; st.best_triw = best; st.bh = th;
                    if (stopped) st.hit = 0;
                }
            }
            if (axis) return false;
        }
    }
    if (!alive) return false;
    RayPrep cr = ray_prepare(lo, ld);
    if (flags & PT_FLAG_EXACT_SLAB) cr.fast = false;
    const TriRay tr = tri_ray_prepare(lo, ld);
    const uint32_t mesh = bu(s, inst + PT_INST_MESH);
    const uint32_t node_off = bu(s, mesh + PT_MESH_NODE_OFF), node_count = bu(s, mesh + PT_MESH_NODE_COUNT), tri_off = bu(s, mesh + PT_MESH_TRI_OFF);
    float limit = __builtin_fminf(st.closest, bound);
    const uint32_t leaf_off = bu(s, mesh + PT_MESH_LEAF_OFF);
    PT_STAT_WALK(lo, ld, bound, st.closest, stop);
    // (bounded searches — light rays, which also stop at the first opaque hit — prune so much of the tree that the walk wins; measured
    // again with the group boxes below: C3 k_shadow_parked 5730 us through the grouped sweep, 5635 through the walk)
    // The mesh sweep reads its leaf list with wave-uniform addresses: every lane that takes it must be in the same mesh.  A table
    // with two walked meshes can resume lanes of both in one wave — those waves walk (same result, lane by lane).
    if (leaf_off != 0u && !(bound < PT_INF) && !(flags & (PT_FLAG_NO_SWEEP | PT_FLAG_NO_MESH_SWEEP)) && !PT_WAVE_ANY(mesh != PT_UNIFORM(mesh) || begin_at != 0u)) {
        // mesh sweep: the leaf-box sweep of world_hit_sweep applied to this mesh, 64 leaves (in pre-order) at a time, each
        // chunk culled by the closest hit the chunks before it left — the same leaves in the same order as the walk below
        const uint32_t leaf_count = PT_UNIFORM(bu(s, mesh + PT_MESH_LEAF_COUNT));
        const bool quick = cr.fast && ld.x != 0.0f && ld.y != 0.0f && ld.z != 0.0f;
        // the settled box tests' triangles in bit order, against the running closest hit; returns true when the search is over (early stop)
        auto triangles = [&](uint64_t hit, uint32_t first) {
            while (hit != 0) {
                const uint32_t k = ctz64(hit);
                hit &= hit - 1;
                const uint32_t t = mu(s, leaf_off + (first + k) * 8u + 3u);
                F4 q0 = mf4(s, t), q1 = mf4(s, t + 4), q2 = mf4(s, t + 8);
                TriHit th;
                if (triangle_test(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tr, 0.0f, st.closest, &th)) {
                    st.closest = th.t; st.best_inst = inst_id; st.best_triw = t; st.bh = th;
                    limit = __builtin_fminf(st.closest, bound);
                    if (inside && __builtin_fminf(__builtin_fminf(th.b0, th.b1), th.b2) >= PT_INSIDE_BARY) { PT_STAT_INSIDE_STOP(); return true; }   // (this mesh is done for this lane; the ray's other leaves are not)
                    if (stop == PT_STOP_ANY) { st.hit = 0; return true; }
                    if (stop == PT_STOP_NONLIGHT && st.closest < bound) {
                        uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                        if (PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : pt_f2u(q0.w)) != PT_TAG_LIGHT) { st.hit = 0; return true; }
                    }
                }
            }
            return false;
        };
        const uint32_t group_off = PT_UNIFORM(bu(s, mesh + PT_MESH_GROUP_OFF));
        if (group_off != 0u) {
            // A bigger mesh (the gem of C3: 302 leaves): the boxes of the groups of PT_MESH_GROUP consecutive leaves first, every lane the
            // same box (wave-uniform addresses); then every lane the leaves of the groups ITS ray enters, in order, a group's triangles
            // right after its boxes.  A group's box holds its leaves' boxes, so a leaf whose box passes AABB::hit is in an entered group
            // (the slab test is monotone under rounding, as for a BVH ancestor); same leaves in the same order as the walk.
            const uint32_t groups = (leaf_count + PT_MESH_GROUP - 1u) / PT_MESH_GROUP;
            static_assert((PT_MESH_SWEEP_MAX + PT_MESH_GROUP - 1) / PT_MESH_GROUP <= 64 && PT_MESH_GROUP <= 32, "one bit per group, one per leaf of a group");
            uint64_t entered = 0;
            float far_leave = -PT_INF; uint32_t far_group = NONE;   // (PT_INSIDE_FIRST_GROUP: the entered group an inside ray leaves last)
            const bool try_first = PT_INSIDE_FIRST_GROUP && inside && quick && !regroup && stop == PT_STOP_NONE;
            const bool rank = PT_INSIDE_FIRST_GROUP && !PT_GROUP_WAVE_MASKS && PT_WAVE_ANY(try_first);   // (wave-uniform: some lane's ray starts inside this body; the wave-mask form of the group boxes keeps no exit distance: no ranking there)
            (void)far_leave;
#if PT_GROUP_WAVE_MASKS && defined(__HIP_DEVICE_COMPILE__)
            {   // (round 5: the group boxes — every lane the same box — decided as wave masks, as the leaf sweep's boxes are: aabb_classify_wave; a group counts as entered when its
                // box is hit OR too close to call, as below)
                const uint64_t q = PT_WAVE_BALLOT(quick), nq = PT_WAVE_BALLOT(!quick);
                const float lim = cull ? limit : PT_INF;
                uint32_t ent_lo = 0u, ent_hi = 0u;
                for (uint32_t g = 0; g < groups; ++g) {
                    const uint32_t e = PT_UNIFORM(group_off + g * 8u);
                    const F4 ga = mf4(s, e), gb = mf4(s, e + 4);
                    float entry = 0.0f;
                    uint64_t ih = 0ull, iu = 0ull;
                    if (PT_UNIFORM(pt_f2u(gb.w)) != 0u) aabb_classify_wave<4>(ga, gb, cr, &entry, &ih, &iu); else aabb_classify_wave<0>(ga, gb, cr, &entry, &ih, &iu);
                    ih &= q; iu = (iu & q) | nq;
                    ih &= ~PT_WAVE_BALLOT(beyond(entry, lim, cr.base));
                    const bool in = PT_WAVE_MEMBER(ih | iu);
                    const uint32_t m = 1u << (g & 31u);
                    if (g < 32u) ent_lo |= in ? m : 0u; else ent_hi |= in ? m : 0u;
                }
                entered = (uint64_t)ent_lo | (uint64_t)ent_hi << 32;
            }
#else
            for (uint32_t g = 0; g < groups; ++g) {
                const uint32_t e = PT_UNIFORM(group_off + g * 8u);
                const F4 ga = mf4(s, e), gb = mf4(s, e + 4);
                float entry = 0.0f, leave = 0.0f;
                int ct = quick ? aabb_classify(ga, gb, cr, PT_UNIFORM(pt_f2u(gb.w)) != 0u, &entry, rank ? &leave : nullptr) : 2;
                if (ct == 1 && cull && beyond(entry, limit, cr.base)) ct = 0;
                entered |= ct != 0 ? 1ull << g : 0ull;
                if (rank) { const float key = PT_FIRST_RANK == 0 ? leave : (PT_FIRST_RANK == 1 ? entry : entry + leave); const bool far = (ct != 0) & (key > far_leave); far_leave = far ? key : far_leave; far_group = far ? g : far_group; }
            }
#endif
            if (regroup) entered = *aux;   // (a resumed ray's own groups; the box tests above were the fresh rays' — the loop's addresses are the wave's)
#if PT_INSIDE_FIRST_GROUP
            // A ray that starts INSIDE this certified convex body leaves it through exactly one triangle, and that triangle's group box reaches at least as far along the ray
            // as the exit point: the entered group that the ray leaves LAST is tried first — without side effects: an acceptance well inside the triangle (the `inside` rule
            // above) is the search's only possible acceptance, committed, and the lane is done with this mesh; an acceptance near an edge spoils the attempt (ties go to
            // pre-order: the lane takes all its groups in order, as if nothing had been tried); no acceptance means none in the ordered search either (the interval only
            // shrinks, and the tests are monotone in it), and the group is dropped.  The choice of the group decides nothing but the time.
            if (rank) {
                PT_KEEP_BRANCH();
                if (try_first && far_group != NONE) {
                    const uint32_t first = far_group * PT_MESH_GROUP, chunk = leaf_count - first < PT_MESH_GROUP ? leaf_count - first : PT_MESH_GROUP;
                    uint32_t hit = 0;
                    for (uint32_t t = 0; t < PT_MESH_GROUP; ++t) {
                        if (t >= chunk) break;
                        const uint32_t e = leaf_off + (first + t) * 8u;
                        F4 ta = mf4(s, e), tb = mf4(s, e + 4);
                        ta.w = pt_u2f(pt_f2u(tb.w) != 0u ? PT_NODE_FLAT : 0u);
                        float entry = 0.0f;
                        const bool box = walk_box(ta, tb, cr, quick, &entry) & !(cull & beyond(entry, limit, cr.base));
                        hit |= box ? 1u << t : 0u;
                    }
                    bool found = false, spoiled = false;
                    while (hit != 0u && !found && !spoiled) {
                        const uint32_t k = (uint32_t)__builtin_ctz(hit);
                        hit &= hit - 1u;
                        const uint32_t t = mu(s, leaf_off + (first + k) * 8u + 3u);
                        const F4 q0 = mf4(s, t), q1 = mf4(s, t + 4), q2 = mf4(s, t + 8);
                        TriHit th;
                        if (triangle_test(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tr, 0.0f, st.closest, &th)) {
                            if (__builtin_fminf(__builtin_fminf(th.b0, th.b1), th.b2) >= PT_INSIDE_BARY) {
                                st.closest = th.t; st.best_inst = inst_id; st.best_triw = t; st.bh = th;
                                limit = __builtin_fminf(st.closest, bound);
                                found = true;
                                PT_STAT_INSIDE_STOP();
                            } else spoiled = true;
                        }
                    }
                    PT_STAT_FIRST_GROUP(found, spoiled);
                    if (found) entered = 0;
                    else if (!spoiled) entered &= ~(1ull << far_group);
                }
            }
#endif
            const uint32_t group_evict = aux != nullptr ? (policy >> 17) & 0x7fu : 0u;
#if PT_SWEEP_FIFO
            // The leaves of the entered groups, per lane — but a lane's triangle tests do not follow its box tests at once: the leaves whose box
            // passed wait in a queue of the lane's own (fourteen 9-bit leaf numbers in two words), and the wave runs a round of triangle tests — one
            // per lane that holds a leaf — only when half its lanes do, when a queue is nearly full, or when no group is left.  In the plain loop a
            // step costs six box tests and as many triangle rounds as the lane with the most hits needs (0.2 of the lanes busy: walk_stats on the
            // gem, 5.7 groups and 7.9 triangles per ray); here the triangle rounds run full.  A lane's leaves keep their order; the closest hit
            // that culls its later boxes is a few triangles older, which only lets through leaves whose triangle cannot be accepted.
            static_assert(PT_MESH_SWEEP_MAX <= 512 && PT_MESH_GROUP <= 8, "nine bits per queued leaf, room for a group's leaves below the fill mark");
            unsigned __int128 fifo = 0;
            uint32_t queued = 0;
            for (;;) {
                if (entered != 0 && queued <= 14u - PT_MESH_GROUP) {
                    const uint32_t g = ctz64(entered);
                    entered &= entered - 1;
                    const uint32_t first = g * PT_MESH_GROUP, chunk = leaf_count - first < PT_MESH_GROUP ? leaf_count - first : PT_MESH_GROUP;
                    uint32_t hit = 0;
#if PT_GROUP_WALK_BOX
                    // (round 5: the leaf boxes of an entered group through the walk's data-flow test — the lanes stand on different leaves, as in a walk step: the thick form
                    // for every lane, the flat form and the exact test under wave-uniform branches — instead of aabb_classify's per-lane nest and a loop over the undecided)
                    for (uint32_t t = 0; t < PT_MESH_GROUP; ++t) {
                        if (t >= chunk) break;
                        const uint32_t e = leaf_off + (first + t) * 8u;
                        F4 ta = mf4(s, e), tb = mf4(s, e + 4);
                        ta.w = pt_u2f(pt_f2u(tb.w) != 0u ? PT_NODE_FLAT : 0u);   // (a leaf-list entry keeps its "flat" flag in [7]; walk_box reads it where a node keeps it)
                        float entry = 0.0f;
                        const bool box = walk_box(ta, tb, cr, quick, &entry) & !(cull & beyond(entry, limit, cr.base));
                        hit |= box ? 1u << t : 0u;
                    }
#else
                    uint32_t unc = 0;
                    for (uint32_t t = 0; t < PT_MESH_GROUP; ++t) {
                        if (t >= chunk) break;
                        const uint32_t e = leaf_off + (first + t) * 8u;
                        const F4 ta = mf4(s, e), tb = mf4(s, e + 4);
                        float entry = 0.0f;
                        int ct = quick ? aabb_classify(ta, tb, cr, pt_f2u(tb.w) != 0u, &entry) : 2;
                        if (ct == 1 && cull && beyond(entry, limit, cr.base)) ct = 0;
                        hit |= ct == 1 ? 1u << t : 0u; unc |= ct == 2 ? 1u << t : 0u;
                    }
                    while (unc != 0u) {
                        const uint32_t k = (uint32_t)__builtin_ctz(unc);
                        unc &= unc - 1u;
                        const uint32_t e = leaf_off + (first + k) * 8u;
                        float entry;
                        PT_STAT(box_exact);
                        if (aabb_hit_exact(mf4(s, e), mf4(s, e + 4), lo, ld, &entry)) hit |= 1u << k;
                    }
#endif
                    while (hit != 0u) {
                        const uint32_t k = (uint32_t)__builtin_ctz(hit);
                        hit &= hit - 1u;
                        fifo |= (unsigned __int128)(first + k) << (9u * queued);
                        ++queued;
                    }
                }
                for (;;) {
                    const uint32_t holders = (uint32_t)__builtin_popcountll(PT_WAVE_BALLOT(queued != 0u));
                    if (holders == 0u) break;
                    const bool groups_left = PT_WAVE_ANY(entered != 0);
                    if (groups_left && holders < PT_SWEEP_FIFO_ROUND && !PT_WAVE_ANY(entered != 0 && queued > 14u - PT_MESH_GROUP)) break;
                    if (queued != 0u) {
                        const uint32_t leaf = (uint32_t)fifo & 511u;
                        fifo >>= 9; --queued;
                        if (triangles(1ull, leaf)) { queued = 0; entered = 0; fifo = 0; }   // (an early stop: this lane's search is over)
                    }
                }
                if (!PT_WAVE_ANY(entered != 0 || queued != 0u)) break;
                if (group_evict != 0u) {
                    const uint32_t busy = (uint32_t)__builtin_popcountll(PT_WAVE_BALLOT(entered != 0 || queued != 0u));
                    if (busy < group_evict) {   // (wave-uniform) the last lanes: their queued triangles, then out with the groups they have left
                        while (queued != 0u) {
                            const uint32_t leaf = (uint32_t)fifo & 511u;
                            fifo >>= 9; --queued;
                            if (triangles(1ull, leaf)) { queued = 0; entered = 0; fifo = 0; }
                        }
                        if (entered != 0) { *cursor = PT_GROUPS_EVICTED; *aux = entered; return true; }
                        break;
                    }
                }
            }
            return false;
#else
            while (entered != 0) {
                const uint32_t g = ctz64(entered);
                entered &= entered - 1;
                const uint32_t first = g * PT_MESH_GROUP, chunk = leaf_count - first < PT_MESH_GROUP ? leaf_count - first : PT_MESH_GROUP;
                uint32_t hit = 0, unc = 0;
                for (uint32_t t = 0; t < PT_MESH_GROUP; ++t) {
                    if (t >= chunk) break;
                    const uint32_t e = leaf_off + (first + t) * 8u;
                    const F4 ta = mf4(s, e), tb = mf4(s, e + 4);
                    float entry = 0.0f;
                    int ct = quick ? aabb_classify(ta, tb, cr, pt_f2u(tb.w) != 0u, &entry) : 2;
                    if (ct == 1 && cull && beyond(entry, limit, cr.base)) ct = 0;
                    hit |= ct == 1 ? 1u << t : 0u; unc |= ct == 2 ? 1u << t : 0u;
                }
                while (unc != 0u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(unc);
                    unc &= unc - 1u;
                    const uint32_t e = leaf_off + (first + k) * 8u;
                    float entry;
                    PT_STAT(box_exact);
                    if (aabb_hit_exact(mf4(s, e), mf4(s, e + 4), lo, ld, &entry)) hit |= 1u << k;
                }
                if (triangles(hit, first)) return false;
            }
            return false;
#endif
        }
        for (uint32_t first = 0; first < leaf_count; first += 64u) {
            const uint32_t chunk = leaf_count - first < 64u ? leaf_count - first : 64u;
            uint32_t hit_lo = 0, hit_hi = 0, unc_lo = 0, unc_hi = 0;
            for (uint32_t t = 0; t < chunk; ++t) {
                const uint32_t e = PT_UNIFORM(leaf_off + (first + t) * 8u);
                const F4 ta = mf4(s, e), tb = mf4(s, e + 4);
                float entry = 0.0f;
                int ct = quick ? aabb_classify(ta, tb, cr, PT_UNIFORM(pt_f2u(tb.w)) != 0u, &entry) : 2;   // ([7]: the test form; two forms here, measured: the five-way switch costs C3 8 %)
                if (ct == 1 && cull && beyond(entry, limit, cr.base)) ct = 0;
                const uint32_t m = 1u << (t & 31u);
                if (t < 32u) { hit_lo |= ct == 1 ? m : 0u; unc_lo |= ct == 2 ? m : 0u; } else { hit_hi |= ct == 1 ? m : 0u; unc_hi |= ct == 2 ? m : 0u; }
            }
            uint64_t hit = (uint64_t)hit_lo | (uint64_t)hit_hi << 32, unc = (uint64_t)unc_lo | (uint64_t)unc_hi << 32;
            while (unc != 0) {
                const uint32_t k = ctz64(unc);
                unc &= unc - 1;
                const uint32_t e = leaf_off + (first + k) * 8u;
                float entry;
                PT_STAT(box_exact);
                if (aabb_hit_exact(mf4(s, e), mf4(s, e + 4), lo, ld, &entry)) hit |= 1ull << k;
            }
            if (triangles(hit, first)) return false;
        }
        return false;
    }
    uint32_t i = begin_at;
    const bool walk_quick = cr.fast && ld.x != 0.0f && ld.y != 0.0f && ld.z != 0.0f;
    PT_STAT_EVENT(7 + stop);   // (tools/walk_stats.py: a walk begins; 5 = a node's box test, 6 = a triangle test)
#if defined(PT_PARKED_EXP) && (PT_PARKED_EXP & 8)
    i = node_count;   // (measurement, tools/phase_costs_parked.sh: a walk's prologue and what follows it, without its loop)
#endif
    const uint32_t evict_below = policy & 0xffu, search_below = (policy >> 8) & 0xffu;
    bool evicted = false;
#if defined(PT_TIMELINE_RAYS) && defined(__HIP_DEVICE_COMPILE__)
    uint32_t tl_steps = 0;
#endif
    uint32_t pending = NONE, pending2 = NONE, pend_node = 0u, pend2_node = 0u;   // (pending2, the node indices: SPEC only)
    for (;;) {
        const uint32_t walking = search_below != 0u ? PT_WAVE_ACTIVE(2u) : 0u;   // (the emulation's lane: "one of two", so every search is cut short)
        while (i < node_count && (pending == NONE || (SPEC && pending2 == NONE))) {
            PT_STAT_EVENT(5);
            PT_TL_STEP();
            F4 a = mf4(s, node_off + i * PT_NODE_WORDS), b = mf4(s, node_off + i * PT_NODE_WORDS + 4);
            uint32_t exit_i = PT_NODE_EXIT(pt_f2u(a.w)), shape = pt_f2u(b.w);
            float entry;
            // (a ray the filtered test does not take — a zero direction component that was not scanned, magnitudes out of range — goes to the exact test at once:
            // the per-axis filtered form stays out of this loop)
            const bool box = walk_box(a, b, cr, walk_quick, &entry) & !(cull & beyond(entry, limit, cr.base));
            if (SPEC) {
                if (shape == PT_NODE_INNER) i = box ? i + 1 : exit_i;
                else {
                    if (box) { if (pending == NONE) { pending = shape; pend_node = i; } else { pending2 = shape; pend2_node = i; } }
                    i = exit_i;
                }
            } else {   // (selects: an inner node entered goes to its first child, anything else to the node's exit; a leaf entered is held)
                const bool inner = shape == PT_NODE_INNER;
                pending = (!inner & box) ? shape : pending;
                i = (inner & box) ? i + 1 : exit_i;
            }
            if (SPEC) {
                // the lanes still without a first leaf (of the lanes in this loop: the others hold two leaves or have no node left)
                const uint32_t searching = (uint32_t)__builtin_popcountll(PT_WAVE_BALLOT(pending == NONE));
                if (searching == 0u || (search_below != 0u && searching < search_below && searching < walking)) break;
            } else if (search_below != 0u) { const uint32_t searching = PT_WAVE_ACTIVE(1u); if (searching < search_below && searching < walking) break; }
        }
        bool over = false;
        if (pending != NONE) {
            PT_STAT_EVENT(6);
            uint32_t t = tri_off + pending * PT_TRI_WORDS;
            F4 q0 = mf4(s, t), q1 = mf4(s, t + 4), q2 = mf4(s, t + 8);
            TriHit th;
            const bool accepted = triangle_test(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tr, 0.0f, st.closest, &th);
            if (accepted) { st.closest = th.t; st.best_inst = inst_id; st.best_triw = t; st.bh = th; limit = __builtin_fminf(st.closest, bound); }   // (the branch of the test's own division)
            // PT_STOP_ANY: any hit ends the search; PT_STOP_NONLIGHT: something opaque in front of every light does (selects, as in sweep_run)
            const uint32_t im = bu(s, inst + PT_INST_MATERIAL);
            const bool opaque = PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : pt_f2u(q0.w)) != PT_TAG_LIGHT;
            over = accepted & ((stop == PT_STOP_ANY) | ((stop == PT_STOP_NONLIGHT) & (st.closest < bound) & opaque));
            st.hit = over ? 0ull : st.hit;
            // (`inside`: the walk of THIS mesh ends at the first interior acceptance — no node left, no leaf held; the ray's other leaves are not touched)
            const bool last = inside && accepted && __builtin_fminf(__builtin_fminf(th.b0, th.b1), th.b2) >= PT_INSIDE_BARY;
            if (last) { PT_STAT_INSIDE_STOP(); }
            i = last ? node_count : i; pending2 = last ? NONE : pending2;
        }
        pending = pending2; pend_node = pend2_node; pending2 = NONE;   // (without SPEC: NONE — every turn begins without a leaf)
        if (over || (i >= node_count && pending == NONE)) break;
        if (evict_below != 0u && PT_WAVE_ACTIVE(0u) < evict_below) { evicted = true; break; }
    }
    PT_TL_DONE();
    PT_STAT_WALK_END(st.hit == 0ull);
    if (evicted) *cursor = (SPEC && pending != NONE) ? pend_node : i;   // (a leaf held untested: its own node, found again on resume)
    return evicted;
}
// A light-sample ray's search may end at a CLOSED mesh without looking at a triangle (round 5; pt_blob.h PT_MESH_INNER_*): if the ray passes through the mesh's
// inner ball at tca > 0 and is beyond the mesh's bounding box — farther from that inside point than the box's diagonal — before `bound`, it crosses the surface in
// between, and the reference's watertight triangle test (mesh.rs:67-198, restated in triangle_test) reports a hit there: a non-light hit in front of every light,
// which is all such a search wants to know (PT_STOP_NONLIGHT, PT_STOP_ANY: the callers read "a light or not", never the occluder's record).  The ball was shrunk by
// 2 % on the host; the test runs in the instance's own space with the un-normalised direction, t is the world ray's parameter.
#ifndef PT_INNER_BALL
#define PT_INNER_BALL 2   /* 0: never; 1: the first ball alone; 2: the further balls too (PT_MESH_MORE_*) */
#endif
// (which searches try it: the light rays — bounded, PT_STOP_NONLIGHT: C3 k_shadow_parked 3783 -> 3558 us.  Environment rays too (PT_STOP_ANY) was measured on C4, whose
// light samples are all of that kind: k_shadow_parked 2904 -> 2929 us — a ray that leaves the monkey's surface for the sky seldom passes through its inside)
#define PT_INNER_BALL_STOP PT_STOP_NONLIGHT
#ifndef PT_INNER_BALL_ANY
#define PT_INNER_BALL_ANY 0   /* 1: environment rays (PT_STOP_ANY) try the balls too */
#endif
PT_HD bool mesh_surely_blocks(const SceneView& s, uint32_t inst, F3 o, F3 d, float bound) {
    if (!PT_INNER_BALL) return false;
    const uint32_t mesh = bu(s, inst + PT_INST_MESH);
    const float r = bf(s, mesh + PT_MESH_INNER_R);
    const uint32_t im = bu(s, inst + PT_INST_MATERIAL);
    if (!(r > 0.0f) || (im != PT_MATERIAL_NONE && PT_MATERIAL_TAG(im) == PT_TAG_LIGHT)) return false;
    F3 lo, ld;
    instance_local_ray(s, inst, o, d, &lo, &ld);
    const float dd = dot(ld, ld), far = 1.01f * bf(s, mesh + PT_MESH_REACH) / pt_sqrt(dd);
    auto through = [&](F3 c, float rr) {
        const F3 oc = sub(c, lo);
        const float tca = dot(oc, ld) / dd;
        const F3 q = sub(oc, mul(ld, tca));
        // (the ball was shrunk by 2 %: the f32 distance of the ray from its centre is right to 1e-6 |oc|, i.e. to a twentieth of that margin for an origin within 1000 radii — farther origins make no claim)
        return (dot(q, q) < rr * rr) & (tca > 0.0f) & (tca + far < bound) & (dot(oc, oc) < 1e6f * rr * rr);
    };
    bool blocks = through(f3(bf(s, mesh + PT_MESH_INNER_C), bf(s, mesh + PT_MESH_INNER_C + 1), bf(s, mesh + PT_MESH_INNER_C + 2)), r);
#if PT_INNER_BALL > 1
    // (the further balls: a ball is an inside point of its own — the same argument; the loop's addresses are the wave's when the rays stand at the same mesh)
    const uint32_t more = bu(s, mesh + PT_MESH_MORE_OFF), n = bu(s, mesh + PT_MESH_MORE_COUNT);
    for (uint32_t k = 0; k < n; ++k) { const F4 b = bf4(s, more + 4u * k); blocks = blocks | through(f3(b.x, b.y, b.z), b.w); }
#endif
    return blocks;
}

// A ray that enters a mesh's bounding box may still miss the mesh by a wide margin — the box's corners are empty (round 5; pt_blob.h PT_MESH_DOP_*).  The host keeps the
// mesh's extent along ten more directions (face and body diagonals: with the box a 26-DOP), widened by 1e-3 of each slab's width; a ray whose segment (0, limit) lies
// outside one of those slabs passes no triangle within 1e-3 of the mesh's size — forty times what the arithmetic of this test and of the triangle test can move anything —
// so every triangle test the reference would run on it fails: the mesh is skipped, no park, no walk.  In the instance's own space, un-normalised direction (t is the world
// ray's).  For every kind of search (a skipped mesh has no hit to offer to any of them).
#ifndef PT_MESH_DOP
#define PT_MESH_DOP 1   /* 0: never; 1: the six face diagonals; 2: the four body diagonals too (measured: the four more cost every kernel more than they skip) */
#endif
// Which searches try it, per kernel family (a translation unit each).  The closest-hit kernels: every ray (k_extend_parked -3 % on C3 and G1, -4 % on C4).  The light-sample
// kernels (PT_MESH_DOP_ONLY_ANY, set by pt_kern_shadow.hip): environment rays only (C4 k_shadow_parked -7 %) — a bounded light ray that crosses a corner of the box leaves
// the BVH after a node or two anyway, and the ten slabs cost its kernel more than those walks (C3 +3 %, G1 +3 %, G2FG +3 %).
#ifndef PT_MESH_DOP_ONLY_ANY
#define PT_MESH_DOP_ONLY_ANY 0
#endif
#define PT_MESH_DOP_TRIES(stop) (!PT_MESH_DOP_ONLY_ANY || (stop) == PT_STOP_ANY)
#ifndef PT_MESH_DOP_SLABS
#define PT_MESH_DOP_SLABS 6   /* how many of the six face-diagonal slabs are tried (2, 4, 6) */
#endif
#ifndef PT_MESH_DOP_TOP
#define PT_MESH_DOP_TOP 1   /* the top-level walk's kernels try it too */
#endif
// Error budget (f32, u = 6e-8): a direction's coordinate of the origin, so = a sum of two or three components, is off by <= 2u L1(o); of the direction, sd, by <= 2u L1(d).  A slab is
// used only if |sd| >= 4e-3 L1(d) — then t = (L - so) / sd (a reciprocal and a product: 3u more) is right to 3e-5 of itself — and only if the origin lies within eight slab widths of
// both planes — then the ray's position along the direction at that t is right to 8 w 3e-5 + 2u L1(o) < 3e-4 w (the host refuses a mesh that lies more than 500 of its own widths
// from its origin: `far` = 0).  The slabs are widened by 1e-3 w on the host.  A direction the ray runs exactly along (sd == 0) separates iff the origin is outside the slab.
PT_HD bool mesh_surely_missed(const SceneView& s, uint32_t inst, F3 o, F3 d, float limit) {
    if (!PT_MESH_DOP) return false;
    const uint32_t dop = bu(s, bu(s, inst + PT_INST_MESH) + PT_MESH_DOP_OFF);
    if (dop == 0u) return false;
    F3 lo, ld;
    instance_local_ray(s, inst, o, d, &lo, &ld);
    const float dmin = 4e-3f * (pt_abs(ld.x) + pt_abs(ld.y) + pt_abs(ld.z));
    // (round-5 advisor: `so` is a sum or difference of the origin's components — small for an origin far away along the slab's own plane, while its rounding error is
    // 2u L1(o) whatever the sum comes to; the budget above wants that below 3e-4 w: a slab is used only by an origin within 250 of its own eight-width window, L1(o) < 2000 w)
    const float l1o = pt_abs(lo.x) + pt_abs(lo.y) + pt_abs(lo.z);
    float t0 = 0.0f, t1 = limit;
    bool apart = false;
    auto slab = [&](uint32_t k, float so, float sd) {   // the ray's coordinate along direction k: so + t sd
        const float L = bf(s, dop + 2u * k), H = bf(s, dop + 2u * k + 1u);
        const float a = L - so, b = H - so, w8 = 8.0f * (H - L);
        const bool flat = sd == 0.0f;
        const bool near = (pt_abs(a) < w8) & (pt_abs(b) < w8) & (l1o < 250.0f * w8);
        const bool usable = (pt_abs(sd) >= dmin) & near;
        const float r = fast_rcp(usable ? sd : 1.0f);
        const float ta = a * r, tb = b * r;
        t0 = __builtin_fmaxf(t0, usable ? __builtin_fminf(ta, tb) : t0);
        t1 = __builtin_fminf(t1, usable ? __builtin_fmaxf(ta, tb) : t1);
        apart = apart | (flat & ((a > 0.0f) | (b < 0.0f)) & near);
    };
    slab(0, lo.x + lo.y, ld.x + ld.y); slab(1, lo.x - lo.y, ld.x - ld.y);
#if PT_MESH_DOP_SLABS > 2
    slab(2, lo.x + lo.z, ld.x + ld.z); slab(3, lo.x - lo.z, ld.x - ld.z);
#endif
#if PT_MESH_DOP_SLABS > 4
    slab(4, lo.y + lo.z, ld.y + ld.z); slab(5, lo.y - lo.z, ld.y - ld.z);
#endif
#if PT_MESH_DOP > 1
    slab(6, lo.x + lo.y + lo.z, ld.x + ld.y + ld.z); slab(7, lo.x + lo.y - lo.z, ld.x + ld.y - ld.z);
    slab(8, lo.x - lo.y + lo.z, ld.x - ld.y + ld.z); slab(9, lo.x - lo.y - lo.z, ld.x - ld.y - ld.z);
#endif
    return apart | (t0 > t1);
}

// Phase 3: the primitive tests of the set bits in pre-order (ties are broken by that order, as in world_hit_walk).  With
// `park_at_walked` the loop returns true when the next bit is a walked mesh instance, leaving the bit set: the caller
// parks the state and resumes with sweep_resume; otherwise walked meshes are walked in line.
// `known_inst`, `known_t`: an instance whose test the caller has run on this very ray already (the nearest light of a light-sample ray,
// nearest_light_hit) and the distance it found: the leaf takes that distance through the interval rule of its shape instead of running
// the test again — the same number through the same comparison.
// PT_SWEEP_ENTRY_REJECT (round 6, EXPERIMENT, off; round-5 verdict item 6 "the entry-distance reject actually built and measured"): phase 1 culls a leaf by the search's
// bound only — the masks do not keep the boxes' entry distances — so phase 3 tests every triangle whose box the ray passes, however far behind the closest hit found
// meanwhile.  With this switch a triangle leaf's box is tested AGAIN once a hit is known (the walk form's rule: beyond(entry, closest)), and the triangle skipped when its box
// begins behind that hit.  Measured on C2: profiles/r6_experiments.md section 4.
#ifndef PT_SWEEP_ENTRY_REJECT
#define PT_SWEEP_ENTRY_REJECT 0
#endif
template <bool WALKS = true>
PT_HD bool sweep_run(const SceneView& s, F3 o, F3 d, const TriRay& wtr, float bound, int stop, SweepState& st, bool park_at_walked,
                     uint32_t known_inst = 0xffffffffu, float known_t = 0.0f, uint32_t inside_inst = 0xffffffffu) {   // (inside_inst: mesh_walk's `inside`, for that instance)
    const uint32_t bits_off = bu(s, PT_HDR_SWEEP_BITS_OFF);
#if PT_SWEEP_ENTRY_REJECT
    const RayPrep erp = ray_prepare(o, d);
    const bool erp_ok = erp.fast & (d.x != 0.0f) & (d.y != 0.0f) & (d.z != 0.0f) & !(bu(s, PT_HDR_FLAGS) & (PT_FLAG_NO_CULL | PT_FLAG_EXACT_SLAB));
#endif
    while (st.hit != 0) {
        const uint32_t k = ctz64(st.hit);
        const F4 be = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS);
        const uint32_t inst = pt_f2u(be.x), triw = pt_f2u(be.y), kf = pt_f2u(be.w);
        if (WALKS && (kf & PT_SWEEP_WALKED)) {  // WALKS = false: the table is known to hold no walked mesh (pure sweep kernels)
            if ((stop == PT_INNER_BALL_STOP || (PT_INNER_BALL_ANY && stop == PT_STOP_ANY)) && mesh_surely_blocks(s, inst, o, d, __builtin_fminf(bound, st.closest))) {   // (no walk: the mesh is closed and the ray goes through its inside)
                st.closest = 0.0f; st.best_inst = kf >> 16; st.best_triw = 0u; st.hit = 0;
                return false;
            }
            if (PT_MESH_DOP_TRIES(stop) && mesh_surely_missed(s, inst, o, d, __builtin_fminf(bound, st.closest))) { st.hit &= st.hit - 1; continue; }   // (through a corner of the mesh's box: nothing to walk for)
            if (park_at_walked) return true;
            st.hit &= st.hit - 1;
            mesh_walk(s, inst, kf >> 16, o, d, bound, stop, st, nullptr, 0u, true, nullptr, (kf >> 16) == inside_inst);
            continue;
        }
        st.hit &= st.hit - 1;
        PT_STAT_EVENT(triw != 0u ? 3 : 4);
        if (triw != 0u) {
            // the copy of the triangle whose vertices are permuted for this ray's dominant axis (kz = 2, 3: the original);
            // the world ray's constants unless the instance is transformed (no copy of the 11-register TriRay)
            const F4 bp = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS + 4);
            TriHit th;
            F4 q0;
            auto test = [&](const TriRay& tr) {
                uint32_t off0 = pt_f2u(bp.z), off1 = pt_f2u(bp.w);
                PT_PIN2(off0, off1);   // (both offsets read, then two selects: the compiler would sink each read into a branch of its own)
                const uint32_t tp = triw + (tr.kz == 0u ? off0 : (tr.kz == 1u ? off1 : 0u));
                q0 = mf4(s, tp);
                const F4 q1 = mf4(s, tp + 4), q2 = mf4(s, tp + 8);
                return triangle_test_permuted(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tr, 0.0f, st.closest, &th);
            };
            bool accepted;
#if PT_SWEEP_ENTRY_REJECT
            if (erp_ok && st.closest < PT_INF && !sweep_leaf_transformed(s, kf)) {
                const uint32_t box = pt_f2u(be.z);
                const F4 ba = bf4(s, box), bb = bf4(s, box + 4);
                const float n0 = __builtin_fminf(approx_fma(ba.x, erp.r.x, erp.nor.x), approx_fma(bb.x, erp.r.x, erp.nor.x));
                const float n1 = __builtin_fminf(approx_fma(ba.y, erp.r.y, erp.nor.y), approx_fma(bb.y, erp.r.y, erp.nor.y));
                const float n2 = __builtin_fminf(approx_fma(ba.z, erp.r.z, erp.nor.z), approx_fma(bb.z, erp.r.z, erp.nor.z));
                if (beyond(slab_entry(n0, n1, n2), st.closest, erp.base)) continue;   // (the box begins behind the closest hit: its triangle cannot be accepted)
            }
#endif
            if (sweep_leaf_transformed(s, kf)) { F3 lo, ld; instance_local_ray(s, inst, o, d, &lo, &ld); const TriRay ltr = tri_ray_prepare(lo, ld); accepted = test(ltr); }
            else accepted = test(wtr);
            {   // (selects, not branches: see triangle_edges)
                const uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                const bool opaque = PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : pt_f2u(q0.w)) != PT_TAG_LIGHT;
                if (accepted) { st.closest = th.t; st.best_inst = kf >> 16; st.best_triw = triw; st.bh = th; }   // (the branch of the test's own division)
                // PT_STOP_ANY: any hit ends the search; PT_STOP_NONLIGHT: something opaque in front of every light does
                const bool over = accepted & ((stop == PT_STOP_ANY) | ((stop == PT_STOP_NONLIGHT) & (st.closest < bound) & opaque));
                st.hit = over ? 0ull : st.hit;
            }
        } else if ((kf >> 16) == known_inst) {
            // rect.rs / disk.rs reject t > t1, sphere.rs accepts t < t1 (the nearer root first; the farther one is beyond it)
            if ((kf & 0xffu) == PT_SHAPE_SPHERE ? known_t < st.closest : !(known_t > st.closest)) {
                st.closest = known_t; st.best_inst = kf >> 16; st.best_triw = 0;
                if (stop == PT_STOP_ANY) st.hit = 0;   // (a light: PT_STOP_NONLIGHT does not end at it)
            }
        } else {
            F3 lo, ld;
            instance_local_ray(s, inst, o, d, &lo, &ld);
            Hit h;
            if (analytic_hit(s, inst, kf & 0xffu, lo, ld, st.closest, &h)) {
                st.closest = h.t; st.best_inst = kf >> 16; st.best_triw = 0;
                if (stop == PT_STOP_ANY) st.hit = 0;
                else if (stop == PT_STOP_NONLIGHT && st.closest < bound) {
                    uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                    if (PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : h.material) != PT_TAG_LIGHT) st.hit = 0;
                }
            }
        }
    }
    return false;
}
// A parked lane: walk the mesh of its lowest set bit, then carry on with phase 3 (it may park again at another walked mesh).  With
// a `policy` that evicts, the walk may be left unfinished (mesh_walk): true then too, the bit still set and `*cursor` where the walk goes on.
template <bool SPEC = false>
PT_HD bool sweep_resume(const SceneView& s, F3 o, F3 d, float bound, int stop, SweepState& st, uint32_t known_inst = 0xffffffffu, float known_t = 0.0f,
                        uint32_t* cursor = nullptr, uint32_t policy = 0u, bool alive = true, uint64_t* aux = nullptr, uint32_t inside_inst = 0xffffffffu) {
    const uint32_t k = alive ? ctz64(st.hit) : 0u;
    const F4 be = bf4(s, bu(s, PT_HDR_SWEEP_BITS_OFF) + k * PT_SWEEP_BIT_WORDS);
    uint32_t inst = pt_f2u(be.x);
    {   // (mesh_walk: a lane that only helps takes the instance of the first lane that has a ray; some lane of the wave has one.  The broadcast
        // runs in uniform control flow: a readlane of a lane that is inactive at that point returns an unspecified value.)
        const uint32_t lead = PT_WAVE_READ(inst, ctz64(PT_WAVE_BALLOT(alive)));
        inst = alive ? inst : lead;
    }
    if (mesh_walk<SPEC>(s, inst, pt_f2u(be.w) >> 16, o, d, bound, stop, st, cursor, policy, alive, aux, alive && (pt_f2u(be.w) >> 16) == inside_inst)) return true;
    if (!alive) return false;
    if (cursor != nullptr) *cursor = 0u;
    st.hit &= st.hit - 1;   // (zero already after an early stop)
    if (st.hit == 0) return false;
    const TriRay wtr = tri_ray_prepare(o, d);
    return sweep_run<true>(s, o, d, wtr, bound, stop, st, true, known_inst, known_t, inside_inst);
}
// ---- the two-level walk, in the parked kernels' protocol (round 3) ------------------------------------------------------------------
// Scenes without a sweep table (more than 64 instances, or PT_FLAG_NO_SWEEP): the top-level tree is walked lane by lane as in world_hit_walk,
// but a lane that reaches a mesh instance whose box it hits PARKS there, and the mesh is walked when 64 such rays have collected —
// mesh_walk with everything the parked kernels give it (full waves, pooled stragglers, short searches, scanned axis rays).  The state is a
// SweepState whose `hit` word holds the walk's place instead of leaf bits: 1 + the top-level node to visit next, 0 = the search is over
// (which is also what mesh_walk's early stop leaves there).  Same boxes, same instances, same order as world_hit_walk: the top level in
// pre-order with the same test and the same culling, every mesh through mesh_walk against the running closest hit.
PT_HD void top_walk_init(SweepState& st) { sweep_state_init(st, 1ull); }
// A ray's place in a parked entry's cursor word when it was EVICTED from the top-level walk (below) rather than parked at a mesh: no mesh walk to finish first.
#define PT_TOP_EVICTED 0xffffffffu
#ifndef PT_TOP_WALK_BOX
#define PT_TOP_WALK_BOX 1   /* the box test of a top-level step as data flow (walk_box, the mesh walk's) instead of the per-lane nest of aabb_hit_node: round 5 */
#endif
// from the state's place on; true = parked: at a mesh instance (the place is that instance's leaf; `park_at_mesh` false: meshes in line; *evicted false), or —
// round 5 — EVICTED (*evicted true, the place is the next node): the walks of a wave's 64 rays differ in length by an order of magnitude (test_bokeh.toml + a floor:
// 32 steps on average, 124 for the slowest lane of a wave), so once fewer than `evict_below` lanes of the wave are still walking, those leave with their place,
// are parked like a ray at a mesh and go on in a later wave of 64 such rays (the mesh walk's policy, mesh_walk: pt_tuning::walk_evict_below).  A ray's own
// sequence of tests is the same; the emulation's one lane leaves at every chance.  0 = never.
// The loop is a while-while (round 5, second step; PT_TOP_WHILE_WHILE=0 builds the single loop it replaces): box steps until the lane HOLDS a leaf whose box it
// hits, then the wave's leaf tests together.  In the single loop every step that found ANY lane a leaf ran the shape test — a square root and two divisions for a
// sphere, ~100 instructions — for that lane alone: with 64 lanes at one leaf per sixteen steps that is nearly every step (G2F: lane utilisation 0.38, 15 000 vector
// instructions per wave).  `search_below`: the inner loop ends once fewer lanes than this are still searching while others hold a leaf (the mesh walk's rule).
#ifndef PT_TOP_WHILE_WHILE
#define PT_TOP_WHILE_WHILE 1
#endif
#ifndef PT_SPHERE_CULL
#define PT_SPHERE_CULL 0   /* 1: top-level nodes that hold untransformed spheres are culled by the closest hit with their certified margin (beyond_sphere, round 6).  Built, bit-identical
                              (4000 fuzz scenes of the many-sphere-lights class), and measured SLOWER on G2F — k_shadow_parked<TOP> 2171 -> 2219 us, k_extend_parked<TOP> 615 -> 655: a
                              pre-order walk seldom holds a near hit when it reaches the far boxes, and the margin (3.5 r + 0.5 % of the distance) is wide against lights a tenth of a
                              unit apart (profiles/r6l_ab_sphere.txt).  0 = such nodes are never culled, as before. */
#endif
// (the mesh walk's early end of the inner loop LOSES here — G2F k_shadow_parked 2313 us with the single loop, 2267 as a pure while-while, 3200 at 16 and 3660 at 32: a lane that
// leaves the search early only waits through the others' leaf tests and searches on — so the kernels pass 0; the emulation's one lane passes 1 and leaves at every step)
#define PT_TOP_SEARCH_BELOW 0u
// (an eviction check INSIDE the search loop — most of G2F's light rays never hold a leaf and so never reach the check behind a leaf test — was measured and lost badly: the
// second exit from the inner loop costs the loop itself, k_shadow_parked 2545 -> 3675 us with eviction off, 2235 -> 2266 at 32: profiles/r5_experiments.md section 10)
#ifndef PT_TOP_EVICT_IN_SEARCH
#define PT_TOP_EVICT_IN_SEARCH 0
#endif
PT_HD bool top_walk_run(const SceneView& s, F3 o, F3 d, float bound, int stop, SweepState& st, bool park_at_mesh, uint32_t evict_below = 0u, bool* evicted = nullptr,
                        uint32_t search_below = 0u) {
    const uint32_t NONE = 0xffffffffu;
    const uint32_t flags = bu(s, PT_HDR_FLAGS);
    const uint32_t top_off = bu(s, PT_HDR_TOP_NODE_OFF), top_count = bu(s, PT_HDR_TOP_NODE_COUNT), inst_off = bu(s, PT_HDR_INSTANCE_OFF);
    const bool cull_top = (flags & (PT_FLAG_NO_TOP_CULL | PT_FLAG_NO_CULL)) == 0;
    const uint32_t margin_off = PT_SPHERE_CULL ? bu(s, PT_HDR_TOP_MARGIN) : 0u;   // (the sphere nodes' certified margins, beyond_sphere; 0: the scene holds no sphere)
    RayPrep wr = ray_prepare(o, d);
    if (flags & PT_FLAG_EXACT_SLAB) wr.fast = false;
    const bool wr_quick = wr.fast && d.x != 0.0f && d.y != 0.0f && d.z != 0.0f;
    if (evicted != nullptr) *evicted = false;
    if (st.hit == 0) return false;
    uint32_t i = (uint32_t)st.hit - 1u;
#if PT_TOP_WHILE_WHILE
    for (;;) {
        // 1 — box steps only, every lane that is still searching; a lane that holds a leaf waits for the others (or for `search_below`)
        uint32_t pending = NONE, pend_node = 0u;
        while (pending == NONE && i < top_count) {
            const F4 a = bf4(s, top_off + i * PT_NODE_WORDS), b = bf4(s, top_off + i * PT_NODE_WORDS + 4);
            const uint32_t exit_i = PT_NODE_EXIT(pt_f2u(a.w)), shape = pt_f2u(b.w);
            float entry;
            bool box = walk_box(a, b, wr, wr_quick, &entry);
            if (margin_off != 0u) box = box & !(cull_top & beyond_sphere(entry, __builtin_fminf(st.closest, bound), wr.base, bf(s, margin_off + i)));   // (wave-uniform: a scene with spheres)
            else box = box & !(cull_top & !(pt_f2u(a.w) & PT_NODE_NO_CULL) & beyond(entry, __builtin_fminf(st.closest, bound), wr.base));
            const bool inner = shape == PT_NODE_INNER;
            pend_node = i;
            pending = (!inner & box) ? shape : NONE;
            i = (inner & box) ? i + 1u : exit_i;
#if !defined(__HIP_DEVICE_COMPILE__)
            if (search_below != 0u && PT_WAVE_ACTIVE(0u) < search_below) break;   // (the emulation only: PT_TOP_SEARCH_BELOW — no scalar compare-and-branch per step in the kernels)
#endif
            // (the wave's last searchers leave from inside the search too: most of G2F's light rays never hold a leaf — 2.2 leaf rounds in a wave's 61 steps — and would never
            // reach the check behind a leaf test, below)
            if (PT_TOP_EVICT_IN_SEARCH && evict_below != 0u && pending == NONE && i < top_count && PT_WAVE_ACTIVE(0u) < evict_below) { st.hit = (uint64_t)i + 1ull; *evicted = true; return true; }
        }
        if (pending == NONE) { if (i >= top_count) break; continue; }   // (done — or the inner loop was left early: search on)
        // 2 — the leaf this lane holds
        const uint32_t inst = inst_off + pending * PT_INST_WORDS, kind = bu(s, inst + PT_INST_KIND);
        if (kind == PT_SHAPE_MESH) {
            // (mesh_surely_blocks is not tried here: in the top-level walk's kernels it cost 2 % — G2FG k_shadow_parked 5896 -> 6022 us — even where no ray could take it)
            if (PT_MESH_DOP_TOP && PT_MESH_DOP_TRIES(stop) && mesh_surely_missed(s, inst, o, d, __builtin_fminf(bound, st.closest))) continue;
            if (park_at_mesh) { st.hit = (uint64_t)pend_node + 1ull; return true; }
            st.hit = (uint64_t)i + 1ull;
            mesh_walk(s, inst, pending, o, d, bound, stop, st);
            if (st.hit == 0) return false;   // (an early stop inside the mesh)
        } else {
            F3 lo, ld;
            instance_local_ray(s, inst, o, d, &lo, &ld);
            Hit h;
            if (analytic_hit(s, inst, kind, lo, ld, st.closest, &h)) {
                st.closest = h.t; st.best_inst = pending; st.best_triw = 0;
                bool over = stop == PT_STOP_ANY;
                if (stop == PT_STOP_NONLIGHT && st.closest < bound) {
                    const uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                    over = PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : h.material) != PT_TAG_LIGHT;   // something opaque in front of every light
                }
                if (over) { st.hit = 0; return false; }
            }
        }
        // (behind a leaf, so that a resumed ray always moves on; a ray on its last node is not worth a parked entry)
        if (evict_below != 0u && i < top_count && PT_WAVE_ACTIVE(0u) < evict_below) { st.hit = (uint64_t)i + 1ull; *evicted = true; return true; }
    }
#else
    while (i < top_count) {
        const F4 a = bf4(s, top_off + i * PT_NODE_WORDS), b = bf4(s, top_off + i * PT_NODE_WORDS + 4);
        const uint32_t exit_i = PT_NODE_EXIT(pt_f2u(a.w)), shape = pt_f2u(b.w);
        float entry;
#if PT_TOP_WALK_BOX
        const bool box = walk_box(a, b, wr, wr_quick, &entry) & !(cull_top & !(pt_f2u(a.w) & PT_NODE_NO_CULL) & beyond(entry, __builtin_fminf(st.closest, bound), wr.base));
#else
        const bool box = aabb_hit_node(a, b, wr, wr_quick, &entry) && !(cull_top && !(pt_f2u(a.w) & PT_NODE_NO_CULL) && beyond(entry, __builtin_fminf(st.closest, bound), wr.base));
#endif
        if (shape == PT_NODE_INNER || !box) i = (shape == PT_NODE_INNER && box) ? i + 1 : exit_i;
        else {
            const uint32_t inst = inst_off + shape * PT_INST_WORDS, kind = bu(s, inst + PT_INST_KIND);
            if (kind == PT_SHAPE_MESH) {
                if (park_at_mesh) { st.hit = (uint64_t)i + 1ull; return true; }
                st.hit = (uint64_t)exit_i + 1ull;
                mesh_walk(s, inst, shape, o, d, bound, stop, st);
                if (st.hit == 0) return false;   // (an early stop inside the mesh)
                i = exit_i;
            } else {
                i = exit_i;
                F3 lo, ld;
                instance_local_ray(s, inst, o, d, &lo, &ld);
                Hit h;
                if (analytic_hit(s, inst, kind, lo, ld, st.closest, &h)) {
                    st.closest = h.t; st.best_inst = shape; st.best_triw = 0;
                    bool over = stop == PT_STOP_ANY;
                    if (stop == PT_STOP_NONLIGHT && st.closest < bound) {
                        const uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                        over = PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : h.material) != PT_TAG_LIGHT;   // something opaque in front of every light
                    }
                    if (over) { st.hit = 0; return false; }
                }
            }
        }
        // (behind a step, so that a resumed ray always moves on; a ray on its last node is not worth a parked entry)
        if (evict_below != 0u && i < top_count && PT_WAVE_ACTIVE(0u) < evict_below) { st.hit = (uint64_t)i + 1ull; *evicted = true; return true; }
    }
#endif
    st.hit = 0;
    return false;
}
// A parked lane: the mesh it stands at (mesh_walk with the wave's policy; true = evicted from it, the place unchanged and `*cursor` where the
// walk goes on), then the top level from behind that instance (true = parked at the next mesh, or evicted from the top-level walk: *cursor = PT_TOP_EVICTED,
// and such a ray has no mesh to finish when it is resumed).
template <bool SPEC = false>
PT_HD bool top_walk_resume(const SceneView& s, F3 o, F3 d, float bound, int stop, SweepState& st, uint32_t* cursor, uint32_t policy, bool alive) {
    const uint32_t top_off = bu(s, PT_HDR_TOP_NODE_OFF), inst_off = bu(s, PT_HDR_INSTANCE_OFF);
    const bool at_mesh = alive && *cursor != PT_TOP_EVICTED;
    const uint64_t mesh_lanes = PT_WAVE_BALLOT(at_mesh);
    if (mesh_lanes != 0ull) {   // (wave-uniform: a wave of rays that were all evicted from the top level — every wave of a scene without meshes — has no mesh walk)
        const uint32_t at = at_mesh ? (uint32_t)st.hit - 1u : 0u;
        const F4 a = bf4(s, top_off + at * PT_NODE_WORDS), b = bf4(s, top_off + at * PT_NODE_WORDS + 4);
        uint32_t shape = pt_f2u(b.w);
        {   // (a lane that only helps: with the instance of the first lane that stands at a mesh — broadcast in uniform control flow, see sweep_resume)
            const uint32_t lead = PT_WAVE_READ(shape, ctz64(mesh_lanes));
            shape = at_mesh ? shape : lead;
        }
        const uint64_t place = st.hit;
        if (at_mesh) st.hit = (uint64_t)PT_NODE_EXIT(pt_f2u(a.w)) + 1ull;
        if (mesh_walk<SPEC>(s, inst_off + shape * PT_INST_WORDS, shape, o, d, bound, stop, st, cursor, policy, at_mesh)) { st.hit = place; return true; }
    }
    if (!alive) return false;
    *cursor = 0u;
    bool evicted = false;
    const bool parked = top_walk_run(s, o, d, bound, stop, st, true, (policy >> 24) & 0xffu, &evicted, (policy >> 8) & 0xffu ? PT_TOP_SEARCH_BELOW : 0u);
    if (evicted) *cursor = PT_TOP_EVICTED;
    return parked;
}

PT_HD bool sweep_finish(const SceneView& s, F3 o, F3 d, const SweepState& st, Hit* out) {
    if (st.best_inst == 0xffffffffu) { out->valid = false; return false; }
    hit_record(s, o, d, st.best_inst, st.best_triw, st.bh, out);
    return true;
}
// ---- phase 3 as independent tests + ordered replay ------------------------------------------------------------------
// The per-lane loop of sweep_run is sequential only through `closest`: a candidate is accepted iff its distance lies in the
// interval that ends at the closest hit so far (triangle: the scaled comparison of mesh.rs:150-158; rect / disk: t <= closest;
// sphere: t < closest, the nearer root first).  Everything else a primitive test computes depends on the ray and the primitive
// alone.  So a candidate can be tested on its own against the unbounded interval — by ANY lane — leaving a record (t, scaled
// t, determinant), and the acceptance decisions are then replayed per ray in leaf order from the records: the same
// comparisons on the same numbers, the same closest hit, ties to the earlier leaf.  The wave pools the candidates of its 64 rays
// and tests them 64 at a time (sweep_run_pooled below): the expensive part runs with full waves, the sequential part is a few
// instructions per candidate.  No early stop: the replay finds the reference's closest hit, of which the early-stop forms only
// use "is it a light / is there one" (DESIGN.md section 5).
struct CandRec { float t, ts, det; uint32_t info; };  // det == 0: never accepted.  info: owner lane | mask bit << 8 | flags
#define PT_CAND_STRICT 0x10000u                        // sphere: accepted iff t < closest (sphere.rs:34-87); the others iff !(t > closest)
PT_HD CandRec cand_none() { CandRec r; r.t = 0.0f; r.ts = 0.0f; r.det = 0.0f; r.info = 0u; return r; }
// a triangle leaf of the table against a ray given by its shear constants (tr.os, tr.kz, tr.sx..sz)
PT_HD CandRec cand_test_triangle(const SceneView& s, uint32_t bits_off, uint32_t k, const TriRay& tr) {
    const F4 be = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS), bp = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS + 4);
    const uint32_t tp = pt_f2u(be.y) + (tr.kz == 0u ? pt_f2u(bp.z) : (tr.kz == 1u ? pt_f2u(bp.w) : 0u));
    const F4 q0 = mf4(s, tp), q1 = mf4(s, tp + 4), q2 = mf4(s, tp + 8);
    CandRec r = cand_none();
    TriEdges g;
    if (!triangle_edges(sub(f3(q0.x, q0.y, q0.z), tr.os), sub(f3(q1.x, q1.y, q1.z), tr.os), sub(f3(q2.x, q2.y, q2.z), tr.os), tr, &g)) return r;
    if (triangle_outside(g.ts, g.det, 0.0f, PT_INF)) return r;
    r.t = g.ts * (1.0f / g.det); r.ts = g.ts; r.det = g.det;
    return r;
}
// a leaf whose test needs the ray itself: an analytic shape, or a triangle of a transformed instance
PT_HD CandRec cand_test_owner(const SceneView& s, uint32_t bits_off, uint32_t k, F3 o, F3 d) {
    const F4 be = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS);
    const uint32_t inst = pt_f2u(be.x), triw = pt_f2u(be.y), kf = pt_f2u(be.w);
    F3 lo, ld;
    instance_local_ray(s, inst, o, d, &lo, &ld);
    if (triw != 0u) return cand_test_triangle(s, bits_off, k, tri_ray_prepare(lo, ld));
    CandRec r = cand_none();
    Hit h;
    PT_STAT_EVENT(4);
    if (analytic_hit(s, inst, kf & 0xffu, lo, ld, PT_INF, &h)) {
        r.t = h.t; r.ts = h.t; r.det = 1.0f;   // rect.rs / disk.rs: rejected iff t > t1 -- the scaled comparison with det = 1
        if ((kf & 0xffu) == PT_SHAPE_SPHERE) r.info = PT_CAND_STRICT;
    }
    return r;
}
PT_HD bool cand_accepts(const CandRec& r, float closest) {
    if (r.det == 0.0f) return false;
    if (r.info & PT_CAND_STRICT) return r.t < closest;
    return !(r.det < 0.0f ? r.ts < closest * r.det : r.ts > closest * r.det);
}
// the winner's place in the running state (barycentrics: the accepted test again, its numbers do not depend on the interval)
PT_HD void cand_winner(const SceneView& s, uint32_t bits_off, uint32_t k, F3 o, F3 d, const TriRay& wtr, float t, SweepState& st) {
    const F4 be = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS), bp = bf4(s, bits_off + k * PT_SWEEP_BIT_WORDS + 4);
    const uint32_t inst = pt_f2u(be.x), triw = pt_f2u(be.y), kf = pt_f2u(be.w);
    st.closest = t; st.best_inst = kf >> 16; st.best_triw = triw;
    if (triw == 0u) return;
    TriRay ltr;
    if (sweep_leaf_transformed(s, kf)) { F3 lo, ld; instance_local_ray(s, inst, o, d, &lo, &ld); ltr = tri_ray_prepare(lo, ld); }
    const TriRay& tr = sweep_leaf_transformed(s, kf) ? ltr : wtr;
    const uint32_t tp = triw + (tr.kz == 0u ? pt_f2u(bp.z) : (tr.kz == 1u ? pt_f2u(bp.w) : 0u));
    const F4 q0 = mf4(s, tp), q1 = mf4(s, tp + 4), q2 = mf4(s, tp + 8);
    triangle_test_permuted(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tr, 0.0f, PT_INF, &st.bh);
}
// One ray on its own (host emulation, PT_FLAG_REPLAY): the records of its set bits, then the replay.
PT_HD void sweep_run_replay(const SceneView& s, F3 o, F3 d, const TriRay& wtr, SweepState& st) {
    const uint32_t bits_off = bu(s, PT_HDR_SWEEP_BITS_OFF);
    const uint64_t owner_mask = (uint64_t)bu(s, PT_HDR_SWEEP_OWNER_MASK) | (uint64_t)bu(s, PT_HDR_SWEEP_OWNER_MASK + 1) << 32;
    CandRec recs[PT_SWEEP_MAX_BITS];
    uint32_t n = 0;
    for (uint64_t m = st.hit; m != 0; m &= m - 1) {
        const uint32_t k = ctz64(m);
        CandRec r;
        if ((owner_mask >> k) & 1ull) r = cand_test_owner(s, bits_off, k, o, d);
        else { PT_STAT_EVENT(3); r = cand_test_triangle(s, bits_off, k, wtr); }
        r.info |= k << 8;
        recs[n++] = r;
    }
    st.hit = 0;
    uint32_t best = 0xffffffffu; float t = PT_INF;
    for (uint32_t i = 0; i < n; ++i)
        if (cand_accepts(recs[i], t)) { t = recs[i].t; best = (recs[i].info >> 8) & 63u; }
    if (best != 0xffffffffu) cand_winner(s, bits_off, best, o, d, wtr, t, st);
}

#if defined(PT_WAVE_KERNELS)   /* defined by pt_engine.hip, after <hip/hip_runtime.h> */
// Inclusive prefix sum over the wave (all 64 lanes must be active): row_shr 1, 2, 4, 8 inside the rows of 16, then row_bcast15
// into rows 1 and 3 and row_bcast31 into rows 2 and 3.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
    uint32_t v = x;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
// Per-wave scratch in LDS, in 32-bit words: 64 ray records of 8 words (o permuted, kz, shear constants), PT_POOL_PAIRS candidate
// records of 4 words, PT_POOL_PAIRS bytes listing the records that are triangle tests.
#define PT_POOL_PAIRS 192u
#define PT_POOL_WORDS (64u * 8u + PT_POOL_PAIRS * 4u + PT_POOL_PAIRS / 4u)
// Phase 3 for the 64 rays of a wave together.  Every lane of the wave must call it (a lane without a ray passes st.hit == 0).
// Rounds: as many rays, in lane order, as have room for all their candidates in the pool; normally one round.
// (EXP: measurement variants that leave parts out, tools/phase_costs.sh; 0 in the product)
template <int EXP = 0>
__device__ __forceinline__ void sweep_run_pooled(const SceneView& s, uint32_t* ws, F3 o, F3 d, const TriRay& wtr, SweepState& st) {
    const uint32_t lane = __lane_id();
    uint4* rays = reinterpret_cast<uint4*>(ws);
    uint4* pool = rays + 128;
    uint8_t* pairs = reinterpret_cast<uint8_t*>(pool + PT_POOL_PAIRS);
    const uint32_t bits_off = bu(s, PT_HDR_SWEEP_BITS_OFF);
    const uint64_t owner_mask = (uint64_t)bu(s, PT_HDR_SWEEP_OWNER_MASK) | (uint64_t)bu(s, PT_HDR_SWEEP_OWNER_MASK + 1) << 32;
    rays[2 * lane] = make_uint4(pt_f2u(wtr.os.x), pt_f2u(wtr.os.y), pt_f2u(wtr.os.z), wtr.kz);
    rays[2 * lane + 1] = make_uint4(pt_f2u(wtr.sx), pt_f2u(wtr.sy), pt_f2u(wtr.sz), 0u);
    uint64_t pending = st.hit;
    st.hit = 0;
    uint32_t best = 0xffffffffu; float closest = PT_INF;
    while (__builtin_amdgcn_ballot_w64(pending != 0) != 0) {
        const uint32_t cnt = (uint32_t)__builtin_popcountll(pending), tcnt = (uint32_t)__builtin_popcountll(pending & ~owner_mask);
        const uint32_t incl = wave_inclusive_scan(cnt | tcnt << 16);
        const bool in = (incl & 0xffffu) <= PT_POOL_PAIRS;   // a prefix of the lanes (the sums do not decrease), never empty (cnt <= 64)
        const uint32_t nin = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
        const uint32_t tri_total = (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(nin - 1u)) >> 16;
        const uint32_t off = (incl & 0xffffu) - cnt;
        if (in && cnt != 0u && !(EXP & 0x40)) {
            // the ray's candidates in leaf order: which bit each record stands for, and the list of the pooled ones
            uint32_t pos = off, tpos = (incl >> 16) - tcnt;
            for (uint64_t m = pending; m != 0; m &= m - 1, ++pos) {
                const uint32_t k = ctz64(m);
                reinterpret_cast<uint32_t*>(pool + pos)[3] = lane | k << 8;
                if (!((owner_mask >> k) & 1ull)) pairs[tpos++] = (uint8_t)pos;
            }
            // the candidates that need the ray itself: tested here, by their owner
            for (uint64_t m = pending & owner_mask; m != 0; m &= m - 1) {
                const uint32_t k = ctz64(m);
                CandRec r = cand_test_owner(s, bits_off, k, o, d);
                pool[off + (uint32_t)__builtin_popcountll(pending & ((1ull << k) - 1ull))] = make_uint4(pt_f2u(r.t), pt_f2u(r.ts), pt_f2u(r.det), r.info | lane | k << 8);
            }
        }
        __threadfence_block();
        // the pooled triangle tests, 64 at a time, whoever the ray belongs to
        for (uint32_t c = 0; c < tri_total && !(EXP & 0x8); c += 64u) {
            const uint32_t idx = c + lane;
            if (idx < tri_total) {
                const uint32_t p = pairs[idx];
                const uint32_t info = reinterpret_cast<const uint32_t*>(pool + p)[3];
                const uint4 r0 = rays[2u * (info & 63u)], r1 = rays[2u * (info & 63u) + 1u];
                TriRay tr;
                tr.os = f3(pt_u2f(r0.x), pt_u2f(r0.y), pt_u2f(r0.z)); tr.kz = r0.w; tr.sx = pt_u2f(r1.x); tr.sy = pt_u2f(r1.y); tr.sz = pt_u2f(r1.z);
                tr.o = tr.os;  // (not used by the permuted test)
                const CandRec r = cand_test_triangle(s, bits_off, (info >> 8) & 63u, tr);
                pool[p] = make_uint4(pt_f2u(r.t), pt_f2u(r.ts), pt_f2u(r.det), info);
            }
        }
        __threadfence_block();
        if (in && cnt != 0u) {
            for (uint32_t i = 0; i < cnt && !(EXP & 0x10); ++i) {
                const uint4 q = pool[off + i];
                CandRec r; r.t = pt_u2f(q.x); r.ts = pt_u2f(q.y); r.det = pt_u2f(q.z); r.info = q.w;
                if (cand_accepts(r, closest)) { closest = r.t; best = (q.w >> 8) & 63u; }
            }
            pending = 0;
        }
        __threadfence_block();  // the records are consumed before a next round overwrites them
    }
    if (EXP & 0x20) { st.closest = closest; st.best_inst = best; return; }
    if (best != 0xffffffffu) cand_winner(s, bits_off, best, o, d, wtr, closest, st);
}
#endif

// Whether the closest hit a sweep found carries a Light-tagged material (the instance's override, else the triangle's own).
PT_HD bool sweep_best_is_light(const SceneView& s, const SweepState& st) {
    const uint32_t inst = bu(s, PT_HDR_INSTANCE_OFF) + st.best_inst * PT_INST_WORDS;
    uint32_t m = bu(s, inst + PT_INST_MATERIAL);
    if (m == PT_MATERIAL_NONE) m = st.best_triw != 0u ? pt_f2u(mf4(s, st.best_triw).w) : PT_MATERIAL_ID(PT_TAG_MATERIAL, 0);
    return PT_MATERIAL_TAG(m) == PT_TAG_LIGHT;
}
// LIGHT_ONLY (light-sample rays): only a light's record is ever read (shadow_ray_contribution) — of any other closest hit the caller
// learns that it exists and that it is no light, and the record (a triangle's vertices, barycentric point and normal) is not built.
// The leaf-mask bits of an instance (its own and its triangle leaves'): what a ray that cannot hit the instance — a light-sample ray that left a certified convex body
// outward, pt_blob.h PT_INST_CONVEX_OUT — drops from its mask before phase 3.
PT_HD uint64_t sweep_instance_mask(const SceneView& s, uint32_t instance) {
    const uint32_t io = bu(s, PT_HDR_INSTANCE_OFF) + instance * PT_INST_WORDS;
    return (uint64_t)bu(s, io + PT_INST_SWEEP_MASK) | (uint64_t)bu(s, io + PT_INST_SWEEP_MASK + 1) << 32;
}
template <bool WALKS = true, bool LIGHT_ONLY = false>
PT_HD bool world_hit_sweep(const SceneView& s, F3 o, F3 d, Hit* out, float bound, int stop, uint32_t known_inst = 0xffffffffu, float known_t = 0.0f, uint32_t skip_inst = 0xffffffffu,
                           uint32_t inside_inst = 0xffffffffu) {
    SweepState st;
    sweep_state_init(st, sweep_masks(s, o, d, bound));
    if (WALKS && skip_inst != 0xffffffffu) st.hit &= ~sweep_instance_mask(s, skip_inst);
    const TriRay wtr = tri_ray_prepare(o, d);
#if !defined(__HIP_DEVICE_COMPILE__)
    if ((bu(s, PT_HDR_FLAGS) & (PT_FLAG_REPLAY | PT_FLAG_SWEEP_WALKS)) == PT_FLAG_REPLAY) { sweep_run_replay(s, o, d, wtr, st); return sweep_finish(s, o, d, st, out); }
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
    if ((bu(s, PT_HDR_FLAGS) & (PT_FLAG_REPLAY | PT_FLAG_SWEEP_WALKS)) == (PT_FLAG_REPLAY | PT_FLAG_SWEEP_WALKS)) {
        // the parked kernels' protocol, lane by lane: park at a walked mesh, resume, and leave the walk at every chance (mesh_walk's eviction)
        uint32_t cursor = 0u;
        bool parked = sweep_run<WALKS>(s, o, d, wtr, bound, stop, st, true, known_inst, known_t, inside_inst);
        uint64_t aux = 0ull;   // (the grouped sweep's group loop too is left at every chance: 2 << 17 against the emulation's one busy lane)
        while (parked) parked = sweep_resume(s, o, d, bound, stop, st, known_inst, known_t, &cursor, 0x201u | PT_WALK_SCAN_AXIS | (2u << 17), true, &aux, inside_inst);
    } else
#endif
    sweep_run<WALKS>(s, o, d, wtr, bound, stop, st, false, known_inst, known_t, inside_inst);
    if (LIGHT_ONLY && st.best_inst != 0xffffffffu && !sweep_best_is_light(s, st)) { out->valid = true; out->material = PT_MATERIAL_ID(PT_TAG_MATERIAL, 0); return true; }
    return sweep_finish(s, o, d, st, out);
}

PT_HD bool world_hit_walk(const SceneView& s, F3 o, F3 d, Hit* out, float bound, int stop) {
    const uint32_t NONE = 0xffffffffu;
    const uint32_t flags = bu(s, PT_HDR_FLAGS);
    const uint32_t top_off = bu(s, PT_HDR_TOP_NODE_OFF), top_count = bu(s, PT_HDR_TOP_NODE_COUNT), inst_off = bu(s, PT_HDR_INSTANCE_OFF);
    const bool exact = (flags & PT_FLAG_EXACT_SLAB) != 0;
    const bool cull_top = (flags & (PT_FLAG_NO_TOP_CULL | PT_FLAG_NO_CULL)) == 0, cull_mesh = (flags & PT_FLAG_NO_CULL) == 0;
    RayPrep wr = ray_prepare(o, d);      // world space; reused after every mesh walk and by untransformed instances
    if (exact) wr.fast = false;
    const TriRay wtr = tri_ray_prepare(o, d);
    RayPrep cr = wr;
    TriRay tr = wtr;
    const bool wr_quick = wr.fast && d.x != 0.0f && d.y != 0.0f && d.z != 0.0f;
    bool cr_quick = wr_quick;  // (of the ray the current level is walked with)
    uint32_t node_off = top_off, node_count = top_count, i = 0;
    uint32_t level_inst = NONE, top_resume = 0, tri_off = 0;
    const uint32_t walk_margin_off = PT_SPHERE_CULL ? bu(s, PT_HDR_TOP_MARGIN) : 0u;
    // `bound`: the caller knows that no hit beyond it can matter (shadow rays: the nearest light hit, see
    // stage_shadow_light); `limit` = min(closest, bound) drives the culling, `closest` keeps the reference's meaning.
    float closest = PT_INF, limit = bound;
    uint32_t best_inst = NONE, best_tri = NONE;
    TriHit bh; bh.t = 0.0f; bh.b0 = bh.b1 = bh.b2 = 0.0f;
    bool done = false;
    PT_STAT_EVENT(0);
    PT_STAT_RAY(o, d);
    for (;;) {
        PT_STAT_EVENT(1);
        // phase 1 — box steps only, until this lane reaches a leaf whose box is hit (or finishes).  All lanes of the wave
        // share these instructions whatever level they are on.
        uint32_t pending = NONE;
        while (!done && pending == NONE) {
            PT_STAT_EVENT(2);
            if (i >= node_count) {
                if (level_inst == NONE) { done = true; break; }
                // the mesh walk is finished: back to the instance level, in world space
                cr = wr; cr_quick = wr_quick;
                node_off = top_off; node_count = top_count; i = top_resume; level_inst = NONE;
                continue;
            }
            // the node array is the top level's (core section) or a mesh's (mesh-data section), lane by lane
            const uint32_t* nb = (level_inst != NONE ? s.m : s.w) + node_off + i * PT_NODE_WORDS;
            F4 a = *reinterpret_cast<const F4*>(nb), b = *reinterpret_cast<const F4*>(nb + 4);
            uint32_t exit_i = PT_NODE_EXIT(pt_f2u(a.w)), shape = pt_f2u(b.w);
            float entry;
            bool box = aabb_hit_node(a, b, cr, cr_quick, &entry);
            if (box) {
                if (level_inst == NONE && walk_margin_off != 0u) box = !(cull_top && beyond_sphere(entry, limit, cr.base, bf(s, walk_margin_off + i)));   // (a top-level node of a scene with spheres)
                else box = !((level_inst != NONE ? cull_mesh : cull_top) && !(pt_f2u(a.w) & PT_NODE_NO_CULL) && beyond(entry, limit, cr.base));
            }
            if (shape == PT_NODE_INNER) { i = box ? i + 1 : exit_i; }
            else { i = exit_i; if (box) pending = shape; }
        }
        if (pending == NONE) break;  // done
        // phase 2 — one leaf per lane: a triangle test inside a mesh, an instance at the top level
        PT_STAT_EVENT(level_inst != NONE ? 3 : 4);
        if (level_inst != NONE) {
            uint32_t t = tri_off + pending * PT_TRI_WORDS;
            F4 q0 = mf4(s, t), q1 = mf4(s, t + 4), q2 = mf4(s, t + 8);
            TriHit th;
            if (triangle_test(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tr, 0.0f, closest, &th)) {
                closest = th.t; best_inst = level_inst; best_tri = pending; bh = th;
                limit = __builtin_fminf(closest, bound);
                if (stop == PT_STOP_ANY) done = true;
                else if (stop == PT_STOP_NONLIGHT && closest < bound) {
                    uint32_t im = bu(s, inst_off + level_inst * PT_INST_WORDS + PT_INST_MATERIAL);
                    uint32_t mat = im != PT_MATERIAL_NONE ? im : pt_f2u(q0.w);
                    if (PT_MATERIAL_TAG(mat) != PT_TAG_LIGHT) done = true;  // something opaque in front of every light
                }
            }
        } else {
            uint32_t inst = inst_off + pending * PT_INST_WORDS;
            uint32_t kind = bu(s, inst + PT_INST_KIND);
            F3 lo, ld;
            instance_local_ray(s, inst, o, d, &lo, &ld);
            if (kind == PT_SHAPE_MESH) {
                uint32_t mesh = bu(s, inst + PT_INST_MESH);
                top_resume = i; level_inst = pending;
                node_off = bu(s, mesh + PT_MESH_NODE_OFF); node_count = bu(s, mesh + PT_MESH_NODE_COUNT); tri_off = bu(s, mesh + PT_MESH_TRI_OFF);
                if (instance_is_transformed(s, inst)) {
                    cr = ray_prepare(lo, ld);
                    if (exact) cr.fast = false;
                    cr_quick = cr.fast && ld.x != 0.0f && ld.y != 0.0f && ld.z != 0.0f;
                    tr = tri_ray_prepare(lo, ld);
                } else { cr = wr; cr_quick = wr_quick; tr = wtr; }
                i = 0;
            } else {
                Hit h;
                if (analytic_hit(s, inst, kind, lo, ld, closest, &h)) {
                    closest = h.t; best_inst = pending; best_tri = NONE;
                    limit = __builtin_fminf(closest, bound);
                    if (stop == PT_STOP_ANY) done = true;
                    else if (stop == PT_STOP_NONLIGHT && closest < bound) {
                        uint32_t im = bu(s, inst + PT_INST_MATERIAL);
                        if (PT_MATERIAL_TAG(im != PT_MATERIAL_NONE ? im : h.material) != PT_TAG_LIGHT) done = true;
                    }
                }
            }
        }
    }
    if (best_inst == NONE) { out->valid = false; return false; }
    uint32_t mesh = bu(s, inst_off + best_inst * PT_INST_WORDS + PT_INST_MESH);
    hit_record(s, o, d, best_inst, best_tri != NONE ? bu(s, mesh + PT_MESH_TRI_OFF) + best_tri * PT_TRI_WORDS : 0u, bh, out);
    return true;
}

// TRAV: PT_TRAV_ANY picks the form at run time (host emulation, probes); the render kernels are instantiated once per form
// so that each keeps its own register budget.
#define PT_TRAV_ANY 0
#define PT_TRAV_WALK 1
#define PT_TRAV_SWEEP 2
PT_HD bool scene_uses_sweep(const SceneView& s) { return bu(s, PT_HDR_SWEEP_OFF) != 0u && !(bu(s, PT_HDR_FLAGS) & PT_FLAG_NO_SWEEP); }
template <int TRAV = PT_TRAV_ANY, bool LIGHT_ONLY = false>
PT_HD bool world_hit(const SceneView& s, F3 o, F3 d, Hit* out, float bound = PT_INF, int stop = PT_STOP_NONE, uint32_t known_inst = 0xffffffffu, float known_t = 0.0f,
                     uint32_t skip_inst = 0xffffffffu, uint32_t inside_inst = 0xffffffffu) {   // (skip_inst: an instance the ray is known not to hit; inside_inst: one it is known to start
                                                                                          // inside of, mesh_walk — optional knowledge: the walk forms do not use it)
    if (TRAV == PT_TRAV_SWEEP) return world_hit_sweep<false, LIGHT_ONLY>(s, o, d, out, bound, stop, known_inst, known_t);
    if (TRAV == PT_TRAV_ANY && scene_uses_sweep(s)) return world_hit_sweep<true, LIGHT_ONLY>(s, o, d, out, bound, stop, known_inst, known_t, skip_inst, inside_inst);
#if !defined(__HIP_DEVICE_COMPILE__)
    if (bu(s, PT_HDR_FLAGS) & PT_FLAG_REPLAY) {
        // (host emulation: the parked kernels' protocol over the top-level tree, lane by lane — park at every mesh, resume, leave the walk at every chance)
        SweepState st;
        top_walk_init(st);
        uint32_t cursor = 0u;
        bool evicted = false;
        bool parked = top_walk_run(s, o, d, bound, stop, st, true, 1u, &evicted, 1u);   // (evict_below / search_below 1 against the emulation's 0 active lanes: the ray leaves at every chance)
        if (evicted) cursor = PT_TOP_EVICTED;
        while (parked) parked = top_walk_resume(s, o, d, bound, stop, st, &cursor, 0x01000201u | PT_WALK_SCAN_AXIS, true);
        if (LIGHT_ONLY && st.best_inst != 0xffffffffu && !sweep_best_is_light(s, st)) { out->valid = true; out->material = PT_MATERIAL_ID(PT_TAG_MATERIAL, 0); return true; }
        return sweep_finish(s, o, d, st, out);
    }
#endif
    return world_hit_walk(s, o, d, out, bound, stop);
}

// One light's own shape test on a world ray against the unbounded interval: what nearest_light_hit runs per light whose box passes, and what the lean
// vertex kernel runs on a light-sample ray of a scene with one light (stage_shade) — ONE helper, so the two cannot drift apart (round-4 advisor).
// `entry`: the light-list entry; for a mesh instance it names the ONE emissive face the entry stands for, whose watertight test runs in instance space with
// the walk's own arithmetic (triangle_test on instance_local_ray's ray, as mesh_walk): the same t, so the search bound is the walk's distance to that face.
// Every emissive face has an entry of its own — a test over all entries is a test over every emissive surface.  (Only h->t and h->valid are set then:
// the callers read nothing else.  A mesh instance named as sweep_run's known light changes nothing there: phase 3 takes the known distance for analytic
// leaves only, and tests a triangle again, with this same arithmetic.)
PT_HD bool light_shape_hit(const SceneView& s, uint32_t inst, uint32_t entry, F3 o, F3 d, Hit* h) {
    F3 l0, l1;
    instance_local_ray(s, inst, o, d, &l0, &l1);
    if (!(s.lacks & PT_SCENE_NO_MESH_LIGHTS) && bu(s, inst + PT_INST_KIND) == PT_SHAPE_MESH) {
        const uint32_t triw = bu(s, bu(s, PT_HDR_LIGHT_FACE_OFF) + entry);
        const F4 q0 = mf4(s, triw), q1 = mf4(s, triw + 4), q2 = mf4(s, triw + 8);
        TriHit th;
        const bool ok = triangle_test(f3(q0.x, q0.y, q0.z), f3(q1.x, q1.y, q1.z), f3(q2.x, q2.y, q2.z), tri_ray_prepare(l0, l1), 0.0f, PT_INF, &th);
        h->valid = ok;
        h->t = ok ? th.t : PT_INF;
        return ok;
    }
    return analytic_hit(s, inst, bu(s, inst + PT_INST_KIND), l0, l1, PT_INF, h);
}

// Nearest hit among the light instances that the reference's walk would test for this ray (an instance is tested iff
// its own leaf box passes AABB::hit; ancestor boxes contain it, and the slab test is monotone under rounding, so they
// pass too).  Returns +inf if no light is hit.  Same arithmetic as the walk, so the distance is the one the walk finds.
PT_HD float nearest_light_hit(const SceneView& s, F3 o, F3 d, uint32_t* which = nullptr) {
    const uint32_t n = bu(s, PT_HDR_LIGHT_COUNT), lo_ = bu(s, PT_HDR_LIGHT_OFF), ln = bu(s, PT_HDR_LIGHT_NODE_OFF), inst_off = bu(s, PT_HDR_INSTANCE_OFF);
    RayPrep wr = ray_prepare(o, d);
    if (bu(s, PT_HDR_FLAGS) & PT_FLAG_EXACT_SLAB) wr.fast = false;
    const bool quick = wr.fast & (d.x != 0.0f) & (d.y != 0.0f) & (d.z != 0.0f);
    const uint64_t q = PT_WAVE_BALLOT(quick), nq = PT_WAVE_BALLOT(!quick);
    float best = PT_INF;
    uint32_t light = 0xffffffffu;
    for (uint32_t k = 0; k < n; ++k) {
        uint32_t node = bu(s, ln + k);
        F4 a = bf4(s, node), b = bf4(s, node + 4);
        // the box decided as wave masks (aabb_classify_wave); the lanes left undecided — and those whose ray the filter does not take — settle it exactly
        float entry = 0.0f;
        uint64_t hb = 0ull, ub = 0ull;
#if defined(__HIP_DEVICE_COMPILE__)
        aabb_classify_wave_by(PT_UNIFORM(PT_NODE_CODE(pt_f2u(a.w))), a, b, wr, &entry, &hb, &ub);
#else
        if (quick) aabb_classify_wave_by(PT_NODE_CODE(pt_f2u(a.w)), a, b, wr, &entry, &hb, &ub);
#endif
        hb &= q; ub = (ub & q) | nq;
        bool inside = PT_WAVE_MEMBER(hb);
        if (ub != 0ull) { PT_KEEP_BRANCH(); if (PT_WAVE_MEMBER(ub)) { PT_STAT(box_exact); inside = aabb_hit_exact(a, b, o, d, &entry); } }
        if (!inside) continue;
        Hit h;
        if (light_shape_hit(s, inst_off + bu(s, lo_ + k) * PT_INST_WORDS, k, o, d, &h) && h.t < best) { best = h.t; light = bu(s, lo_ + k); }
    }
    if (which != nullptr) *which = light;   // (the instance that gave the distance; 0xffffffff: none)
    return best;
}

// ---------------------------------------------------------------- sampling helpers (math crate)
PT_HD F3 random_cosine_direction(float u, float v) {
    float z = pt_sqrt(1.0f - v);
    float phi = 2.0f * PT_PI * u;
    float sn, cs; pt_sincos(phi, &sn, &cs);
    float r = pt_sqrt(v);
    return f3(cs * r, sn * r, z);
}
PT_HD F3 random_on_unit_sphere(float x, float y) {
    float phi = x * 2.0f * PT_PI;
    float z = y * 2.0f - 1.0f;
    float r = pt_sqrt(1.0f - z * z);
    float sn, cs; pt_sincos(phi, &sn, &cs);
    return f3(r * cs, r * sn, z);
}
PT_HD F3 random_in_unit_disk(float x, float y) {
    float u = x * PT_PI * 2.0f;
    float v = pt_sqrt(y);
    float sn, cs; pt_sincos(u, &sn, &cs);
    return f3(cs * v, sn * v, 0.0f);
}
// Sample1D::choose
PT_HD bool choose_first(float* x, float split) {
    if (*x < split) { *x = *x / split; return true; }
    *x = (*x - split) / (1.0f - split);
    return false;
}
PT_HD F3 uv_to_direction(float u, float v) {
    float theta = (u - 0.5f) * 2.0f * PT_PI;
    float phi = v * PT_PI;
    float st, ct, sp, cp;
    pt_sincos(theta, &st, &ct);
    pt_sincos(phi, &sp, &cp);
    return f3(sp * ct, sp * st, cp);
}
PT_HD void direction_to_uv(F3 d, float* u, float* v) {
    float theta = pt_atan2(d.y, d.x);
    float phi = pt_acos(d.z);
    *u = theta / 2.0f / PT_PI + 0.5f;
    *v = phi / PT_PI;
}

// ---------------------------------------------------------------- GGX (src/materials/ggx.rs:3-180)
PT_HD F3 reflect(F3 wi, F3 n) { F3 w = neg(wi); return normalize(sub(w, mul(n, 2.0f * dot(w, n)))); }
PT_HD bool refract(F3 wi, F3 n, float eta, F3* out) {
    float cos_i = dot(wi, n);
    float sin2_i = pt_max(1.0f - cos_i * cos_i, 0.0f);
    float sin2_t = eta * eta * sin2_i;
    if (sin2_t >= 1.0f) return false;
    float cos_t = pt_sqrt(1.0f - sin2_t);
    *out = normalize(add(mul(neg(wi), eta), mul(n, eta * cos_i - cos_t)));
    return true;
}
PT_HD float fresnel_dielectric(float eta_i, float eta_t, float cos_i) {
    cos_i = pt_clamp(cos_i, -1.0f, 1.0f);
    if (cos_i < 0.0f) { cos_i = -cos_i; float t = eta_i; eta_i = eta_t; eta_t = t; }
    float sin_t = eta_i / eta_t * pt_sqrt(pt_max(0.0f, 1.0f - cos_i * cos_i));
    float cos_t = pt_sqrt(pt_max(0.0f, 1.0f - sin_t * sin_t));
    float ei_ct = eta_i * cos_t, et_ci = eta_t * cos_i, ei_ci = eta_i * cos_i, et_ct = eta_t * cos_t;
    float r_par = (et_ci - ei_ct) / (et_ci + ei_ct);
    float r_perp = (ei_ci - et_ct) / (ei_ci + et_ct);
    return (r_par * r_par + r_perp * r_perp) / 2.0f;
}
PT_HD float fresnel_conductor(float eta_i, float eta_t, float k_t, float c) {
    c = pt_clamp(c, -1.0f, 1.0f);
    if (c < 0.0f) { c = -c; float t = eta_i; eta_i = eta_t; eta_t = t; }
    float eta = eta_t / eta_i, etak = k_t / eta_i;
    float c2 = c * c, s2 = 1.0f - c2;
    float eta2 = eta * eta, etak2 = etak * etak;
    float t0 = eta2 - etak2 - s2;
    float a2plusb2 = pt_sqrt(t0 * t0 + eta2 * etak2 * 4.0f);
    float t1 = a2plusb2 + c2;
    float a = pt_sqrt((a2plusb2 + t0) * 0.5f);
    float t2 = a * c * 2.0f;
    float rs = (t1 - t2) / (t1 + t2);
    float t3 = a2plusb2 * c2 + s2 * s2;
    float t4 = t2 * s2;
    float rp = rs * (t3 - t4) / (t3 + t4);
    return (rs + rp) / 2.0f;
}
PT_HD float ggx_d(float alpha, F3 wm) {
    float sx = wm.x / alpha, sy = wm.y / alpha;
    float t = wm.z * wm.z + sx * sx + sy * sy;
    float a2 = alpha * alpha, t2 = t * t;
    return 1.0f / (PT_PI * (a2 * t2));
}
PT_HD float ggx_lambda(float alpha, F3 w) {
    if (w.z == 0.0f) return 0.0f;
    float a2 = alpha * alpha;
    float c = 1.0f + (a2 * (w.x * w.x) + a2 * (w.y * w.y)) / (w.z * w.z);
    return pt_sqrt(c) * 0.5f - 0.5f;
}
PT_HD float ggx_g(float alpha, F3 wi, F3 wo) { return 1.0f / (1.0f + ggx_lambda(alpha, wi) + ggx_lambda(alpha, wo)); }
PT_HD float ggx_vnpdf(float alpha, F3 wi, F3 wh) {
    float inv_gl = 1.0f + ggx_lambda(alpha, wi);
    return (ggx_d(alpha, wh) * pt_abs(dot(wi, wh))) / (inv_gl * pt_abs(wi.z));
}
PT_HD float ggx_vnpdf_no_d(float alpha, F3 wi, F3 wh) {
    return pt_abs(dot(wi, wh) / ((1.0f + ggx_lambda(alpha, wi)) * wi.z));
}
PT_HD F3 sample_vndf(float alpha, F3 wi, float x, float y) {
    F3 v = normalize(f3(alpha * wi.x, alpha * wi.y, wi.z));
    F3 t1 = (v.z < 0.9999f) ? normalize(cross(v, f3(0, 0, 1))) : f3(1, 0, 0);
    F3 t2 = cross(t1, v);
    float a = 1.0f / (1.0f + v.z);
    float r = pt_sqrt(x);
    float phi = (y < a) ? (y / a * PT_PI) : (PT_PI + (y - a) / (1.0f - a) * PT_PI);
    float sp, cp; pt_sincos(phi, &sp, &cp);
    float p1 = r * cp;
    float p2 = r * sp * ((y < a) ? 1.0f : v.z);
    float value = 1.0f - p1 * p1 - p2 * p2;
    F3 n = add(add(mul(t1, p1), mul(t2, p2)), mul(v, pt_sqrt(pt_max(value, 0.0f))));
    return normalize(f3(alpha * n.x, alpha * n.y, pt_max(n.z, 0.0f)));
}
PT_HD F3 sample_wh(float alpha, F3 wi, float x, float y) {
    bool flip = wi.z < 0.0f;
    F3 wh = sample_vndf(alpha, flip ? neg(wi) : wi, x, y);
    return flip ? neg(wh) : wh;
}
PT_HD float ggx_reflectance(bool metallic, float eo, float ei, float k, float c) {
    return metallic ? fresnel_conductor(eo, ei, k, c) : fresnel_dielectric(eo, ei, c);
}
PT_HD float ggx_reflectance_probability(bool metallic, float eo, float ei, float k, float c) {
    return metallic ? 1.0f : pt_clamp(fresnel_dielectric(eo, ei, c), 0.0f, 1.0f);
}
PT_HD float ggx_eta_rel(float eo, float ei, F3 wi) { return (wi.z < 0.0f) ? eo / ei : ei / eo; }
// transmission lobe, TransportMode::Importance (ggx.rs:310-376 and 476-551)
PT_HD void ggx_transmission(float alpha, bool metallic, float eo, float ei, float kappa, F3 wi, F3 wo, F3 wh, float g,
                            float* transmission, float* transmission_pdf) {
    float eta_rel = ggx_eta_rel(eo, ei, wi);
    float ggxg = ggx_g(alpha, wi, wo);
    float partial = ggx_vnpdf_no_d(alpha, wi, wh);
    float ndotv = dot(wi, wh), ndotl = dot(wo, wh);
    float sqrt_denom = ndotv + eta_rel * ndotl;
    float eta_rel2 = eta_rel * eta_rel;
    float dwh_dwo1 = ndotl / (sqrt_denom * sqrt_denom);
    float dwh_dwo2 = eta_rel2 * dwh_dwo1;
    dwh_dwo1 = dwh_dwo2;  // Importance mode
    float ggxd = ggx_d(alpha, wh);
    float weight = ggxd * ggxg * ndotv * dwh_dwo1 / g;
    *transmission_pdf = pt_abs(ggxd * partial * dwh_dwo2);
    float inv_reflectance = 1.0f - ggx_reflectance(metallic, eo, ei, kappa, ndotv);
    *transmission = metallic ? 0.0f : inv_reflectance * pt_abs(weight);
}

// ---------------------------------------------------------------- Material<f32,f32>
// The spectral inputs of a material at one vertex (same lambda, same uv for the BSDF sample and every light-sample
// evaluation): evaluated once.  The reference re-evaluates its curves in every call (lambertian.rs:25,62; ggx.rs:279-285,
// 409-417); the values are identical, so this changes nothing but the instruction count.
struct MatEval { uint32_t kind; bool metallic; float alpha; float refl; float ei, eo, kappa; };
// GGX = false (here and below): the caller knows the scene holds no GGX material, and the microfacet code is compiled out of its kernel.
template <bool GGX = true>
PT_HD MatEval material_prepare(const SceneView& s, uint32_t m, float lambda, float u, float v) {
    MatEval e;
    e.kind = bu(s, m + PT_MAT_KIND); e.metallic = false; e.alpha = 0.0f; e.refl = 0.0f; e.ei = e.eo = e.kappa = 0.0f;
    if (e.kind == PT_MATERIAL_LAMBERTIAN) e.refl = pt_min(texstack_eval(s, bu(s, m + PT_MAT_TEXSTACK), lambda, u, v), 1.0f);
    else if (GGX && e.kind == PT_MATERIAL_PASSTHROUGH) e.refl = curve_eval(s, bu(s, m + PT_MAT_BOUNCE), lambda);   // PassthroughFilter::color, unclamped (passthrough.rs:36)
    else if (!GGX || e.kind != PT_MATERIAL_GGX) e.refl = pt_clamp(curve_eval(s, bu(s, m + PT_MAT_BOUNCE), lambda), 0.0f, 1.0f);
    else {
        e.alpha = bf(s, m + PT_MAT_ALPHA);
        e.metallic = bu(s, m + PT_MAT_METALLIC) != 0;
        e.ei = curve_eval(s, bu(s, m + PT_MAT_ETA), lambda); e.eo = curve_eval(s, bu(s, m + PT_MAT_ETA_O), lambda);
        e.kappa = e.metallic ? curve_eval(s, bu(s, m + PT_MAT_KAPPA), lambda) : 0.0f;
    }
    return e;
}

// The same for the N wavelengths of a hero-wavelength path: what does not depend on the wavelength once, the spectral values per k.
template <int N> struct MatEvalN { uint32_t kind; bool metallic; float alpha; float refl[N], ei[N], eo[N], kappa[N]; };
template <int N, bool GGX = true>
PT_HD MatEvalN<N> material_prepare_n(const SceneView& s, uint32_t m, const float (&lambda)[N], float u, float v) {
    MatEvalN<N> e;
    e.kind = bu(s, m + PT_MAT_KIND); e.metallic = false; e.alpha = 0.0f;
    for (int k = 0; k < N; ++k) e.refl[k] = e.ei[k] = e.eo[k] = e.kappa[k] = 0.0f;
    PT_ROLLED for (int k = 0; k < N; ++k) {
        const MatEval one = material_prepare<GGX>(s, m, pl_get<N>(lambda, k), u, v);
        e.metallic = one.metallic; e.alpha = one.alpha;
        pl_set<N>(e.refl, k, one.refl);
        if (GGX) { pl_set<N>(e.ei, k, one.ei); pl_set<N>(e.eo, k, one.eo); pl_set<N>(e.kappa, k, one.kappa); }
    }
    return e;
}
template <int N> PT_HD MatEval material_at(const MatEvalN<N>& e, int k) {
    MatEval one; one.kind = e.kind; one.metallic = e.metallic; one.alpha = e.alpha;
    one.refl = pl_get<N>(e.refl, k); one.ei = pl_get<N>(e.ei, k); one.eo = pl_get<N>(e.eo, k); one.kappa = pl_get<N>(e.kappa, k);
    return one;
}

// Material::bsdf (lambertian.rs:16-33, diffuse_light.rs:29-45, sharp_light.rs:43-60, ggx.rs:256-400)
template <bool GGX = true>
PT_HD void material_bsdf_p(const MatEval& e, F3 wi, F3 wo, float* f_out, float* pdf_out) {
    if (GGX && e.kind == PT_MATERIAL_PASSTHROUGH) { *f_out = e.refl / pt_abs(wo.z); *pdf_out = 1.0f; return; }   // passthrough.rs:27-38 (the GGX-free kernel forms never see one)
    if (!GGX || e.kind != PT_MATERIAL_GGX) {
        if (wo.z * wi.z > 0.0f) { *f_out = e.refl / PT_PI; *pdf_out = pt_abs(wo.z) / PT_PI; }
        else { *f_out = 0.0f; *pdf_out = 0.0f; }
        return;
    }
    float alpha = e.alpha; bool metallic = e.metallic; float ei = e.ei, eo = e.eo, kappa = e.kappa;
    wi = normalize(wi);
    bool same_hemisphere = wi.z * wo.z > 0.0f;
    float g = pt_abs(wi.z * wo.z);
    if (g == 0.0f) { *f_out = 0.0f; *pdf_out = 0.0f; return; }
    float cos_i = wi.z;
    float glossy = 0.0f, transmission = 0.0f, glossy_pdf = 0.0f, transmission_pdf = 0.0f;
    if (same_hemisphere) {
        F3 wh = normalize(add(wo, wi));
        if (wh.z < 0.0f) wh = neg(wh);
        float ndotv = dot(wi, wh);
        float refl = ggx_reflectance(metallic, eo, ei, kappa, ndotv);
        float ggxd = ggx_d(alpha, wh), ggxg = ggx_g(alpha, wi, wo);
        glossy = refl * (0.25f / g) * ggxd * ggxg;
        glossy_pdf = (pt_abs(ndotv) == 0.0f) ? 0.0f : ggx_vnpdf(alpha, wi, wh) * 0.25f / pt_abs(ndotv);
    } else if (!metallic) {
        float eta_rel = ggx_eta_rel(eo, ei, wi);
        F3 wh = normalize(add(wi, mul(wo, eta_rel)));
        if (wh.z < 0.0f) wh = neg(wh);
        ggx_transmission(alpha, metallic, eo, ei, kappa, wi, wo, wh, g, &transmission, &transmission_pdf);
    }
    float rp = ggx_reflectance_probability(metallic, eo, ei, kappa, cos_i);
    *f_out = glossy + transmission;
    *pdf_out = rp * glossy_pdf + (1.0f - rp) * transmission_pdf;
}

// Material::generate_and_evaluate (lambertian.rs:50-66, diffuse_light.rs:60-76, sharp_light.rs:183-198, ggx.rs:401-590)
template <bool GGX = true>
PT_HD void material_sample_p(const MatEval& e, float sx, float sy, F3 wi, float* f_out, F3* wo_out, float* pdf_out) {
    if (GGX && e.kind == PT_MATERIAL_PASSTHROUGH) { *f_out = e.refl / pt_abs(wi.z); *wo_out = neg(wi); *pdf_out = 1.0f; return; }   // passthrough.rs:55-68
    if (!GGX || e.kind != PT_MATERIAL_GGX) {
        F3 d = mul(random_cosine_direction(sx, sy), pt_signum(wi.z));
        *f_out = e.refl / PT_PI; *wo_out = d; *pdf_out = pt_abs(d.z) / PT_PI;
        return;
    }
    float alpha = e.alpha; bool metallic = e.metallic; float ei = e.ei, eo = e.eo, kappa = e.kappa;
    F3 wh = normalize(sample_wh(alpha, wi, sx, sy));
    float refl_prob = ggx_reflectance_probability(metallic, eo, ei, kappa, dot(wh, wi));
    bool did_reflect = false;
    F3 wo;
    if (sx <= refl_prob) {
        did_reflect = true; wo = reflect(wi, wh);
    } else {
        float eta_rel = 1.0f / ggx_eta_rel(eo, ei, wi);
        if (!refract(wi, wh, eta_rel, &wo)) { did_reflect = true; wo = reflect(wi, wh); }
    }
    float g = pt_abs(wi.z * wo.z);
    if (g == 0.0f) { *f_out = 0.0f; *wo_out = wo; *pdf_out = 0.0f; return; }
    float cos_i;
    float glossy = 0.0f, transmission = 0.0f, glossy_pdf = 0.0f, transmission_pdf = 0.0f;
    if (did_reflect) {
        cos_i = dot(wi, wh);
        float refl = ggx_reflectance(metallic, eo, ei, kappa, cos_i);
        float ggxd = ggx_d(alpha, wh), ggxg = ggx_g(alpha, wi, wo);
        glossy = refl * (0.25f / g) * ggxd * ggxg;
        glossy_pdf = (pt_abs(cos_i) == 0.0f) ? 0.0f : ggx_vnpdf(alpha, wi, wh) * 0.25f / pt_abs(cos_i);
    } else {
        if (wh.z < 0.0f) wh = neg(wh);
        cos_i = dot(wi, wh);
        ggx_transmission(alpha, metallic, eo, ei, kappa, wi, wo, wh, g, &transmission, &transmission_pdf);
    }
    float rp = ggx_reflectance_probability(metallic, eo, ei, kappa, cos_i);
    *f_out = glossy + transmission;
    *wo_out = wo;
    *pdf_out = rp * glossy_pdf + (1.0f - rp) * transmission_pdf;
}
PT_HD void material_bsdf(const SceneView& s, uint32_t m, float lambda, float u, float v, F3 wi, F3 wo, float* f_out, float* pdf_out) {
    MatEval e = material_prepare(s, m, lambda, u, v);
    material_bsdf_p(e, wi, wo, f_out, pdf_out);
}
PT_HD void material_sample(const SceneView& s, uint32_t m, float lambda, float u, float v, float sx, float sy, F3 wi,
                           float* f_out, F3* wo_out, float* pdf_out) {
    MatEval e = material_prepare(s, m, lambda, u, v);
    material_sample_p(e, sx, sy, wi, f_out, wo_out, pdf_out);
}

// Material::emission (diffuse_light.rs:123-133, sharp_light.rs:138-150, 202-204)
PT_HD float material_emission(const SceneView& s, uint32_t m, float lambda, F3 wi) {
    uint32_t kind = bu(s, m + PT_MAT_KIND);
    if (kind != PT_MATERIAL_DIFFUSE_LIGHT && kind != PT_MATERIAL_SHARP_LIGHT) return 0.0f;
    uint32_t sided = bu(s, m + PT_MAT_SIDEDNESS);
    float cosine = wi.z;
    bool on = (cosine > 0.0f && sided == PT_SIDED_FORWARD) || (cosine < 0.0f && sided == PT_SIDED_REVERSE) || sided == PT_SIDED_DUAL;
    if (!on) return 0.0f;
    float e = curve_eval(s, bu(s, m + PT_MAT_EMIT), lambda);
    if (kind == PT_MATERIAL_DIFFUSE_LIGHT) return e / PT_PI;
    float sharpness = bf(s, m + PT_MAT_SHARPNESS);
    float inner = (sharpness + 1.0f) * pt_pow(pt_abs(wi.z), sharpness) / 2.0f / PT_PI;
    return e * inner;
}
PT_HD uint32_t material_record(const SceneView& s, uint32_t material_id) {
    return bu(s, PT_HDR_MATERIAL_OFF) + PT_MATERIAL_INDEX(material_id) * PT_MAT_WORDS;
}

// ---------------------------------------------------------------- participating media (src/mediums; the medium-aware walk only)
PT_HD float phase_hg(float cos_theta, float g) {   // hg.rs:5-15
    float denom = 1.0f + g * g + 2.0f * g * cos_theta;
    return (1.0f - g * g) / (denom * pt_sqrt(denom) * 2.0f * (2.0f * PT_PI));
}
PT_HD float rayleigh_sigma_s(const SceneView& s, uint32_t m, float lambda) {   // rayleigh.rs:24-40
    float n = curve_eval(s, bu(s, m + PT_MED_IOR), lambda), n2 = n * n;
    float q = (n2 - 1.0f) / (n2 + 2.0f), ior_factor = q * q;
    float r = 1.0f / (lambda / 1000.0f), r2 = r * r, lambda_factor = r2 * r2;
    return ior_factor * bf(s, m + PT_MED_CORRECTIVE) * lambda_factor;
}
PT_HD uint32_t medium_record(const SceneView& s, uint32_t medium_id) { return bu(s, PT_HDR_MEDIUM_OFF) + (medium_id - 1u) * PT_MEDIUM_WORDS; }
// The wavelength-only part of a medium, evaluated once per vertex: sigma_s (free flight), sigma_t (transmittance), g
struct MediumEval { uint32_t kind; float sigma_s, sigma_t, g; };
PT_HD MediumEval medium_prepare(const SceneView& s, uint32_t m, float lambda) {
    MediumEval e; e.kind = bu(s, m + PT_MED_KIND); e.g = 0.0f;
    if (e.kind == PT_MEDIUM_HG) {
        e.sigma_s = curve_eval(s, bu(s, m + PT_MED_SIGMA_S), lambda);
        e.sigma_t = curve_eval(s, bu(s, m + PT_MED_SIGMA_A), lambda) + e.sigma_s;   // hg.rs:35-37
        e.g = curve_eval(s, bu(s, m + PT_MED_G), lambda) + 0.001f - 1.0f;         // hg.rs:69
    } else { e.sigma_s = rayleigh_sigma_s(s, m, lambda); e.sigma_t = e.sigma_s; }
    return e;
}
PT_HD float medium_tr(const MediumEval& e, F3 p0, F3 p1) { return pt_exp(-e.sigma_t * norm(sub(p1, p0))); }   // hg.rs:112-115, rayleigh.rs:96-99
// Medium::sample with tmax = inf: hg.rs:96-111 (weight tr), rayleigh.rs:100-113 (weight tr * sigma_s)
PT_HD void medium_sample(const MediumEval& e, F3 o, F3 d, float x, F3* point, float* weight) {
    float dist = -pt_ln(1.0f - x) / e.sigma_s;
    *point = add(o, mul(d, dist));
    float tr = medium_tr(e, o, *point);
    *weight = e.kind == PT_MEDIUM_HG ? tr : tr * e.sigma_s;
}
// Medium::sample_p: hg.rs:68-95, rayleigh.rs:57-95
PT_HD F3 medium_sample_p(const MediumEval& e, F3 wi, float sx, float sy, float* pdf) {
    Frame frame = frame_from_normal(wi);
    float sn, cs;
    if (e.kind == PT_MEDIUM_HG) {
        float g = e.g, cos_theta;
        if (pt_abs(g) < 0.001f) cos_theta = 1.0f - 2.0f * sx;
        else { float sqr = (1.0f - g * g) / (1.0f + g - 2.0f * g * sx); cos_theta = -(1.0f + g * g - sqr * sqr) / (2.0f * g); }
        float sin_theta = pt_sqrt(pt_max(0.0f, 1.0f - cos_theta * cos_theta));
        pt_sincos((2.0f * PT_PI) * sy, &sn, &cs);
        *pdf = phase_hg(cos_theta, g);
        return to_world(frame, f3(sin_theta * cs, sin_theta * sn, cos_theta));
    }
    float x = sx; bool flipped = choose_first(&x, 0.5f);
    float z = 2.0f * (2.0f * x - 1.0f);
    float right = pt_sqrt(z * z + 1.0f);
    float cos_theta = pt_cbrt(z + right) + pt_cbrt(z - right);
    float sin_theta = pt_sqrt(1.0f - cos_theta * cos_theta) * (flipped ? 1.0f : -1.0f);
    pt_sincos(sy * (2.0f * PT_PI), &sn, &cs);
    *pdf = 3.0f * (1.0f + cos_theta * cos_theta) / 8.0f;
    return to_world(frame, f3(sn * sin_theta, cs * sin_theta, cos_theta));
}
// The list of tracked mediums (utils.rs:731): at most four ids in one word, ascending, zero bytes behind them
PT_HD uint32_t mediums_remove(uint32_t list, uint32_t id) {   // the first occurrence (:944-951)
    for (uint32_t i = 0; i < 4u; ++i)
        if (((list >> (8u * i)) & 0xffu) == id) {
            const uint32_t low = list & ((1u << (8u * i)) - 1u), high = i == 3u ? 0u : (list >> (8u * (i + 1u))) << (8u * i);
            return low | high;
        }
    return list;
}
PT_HD uint32_t mediums_add(uint32_t list, uint32_t id, uint32_t* dropped = nullptr) {      // push + sort_unstable (:965-968); a fifth entry is dropped — and counted (pt_profile::stage_items[5])
    if ((list >> 24) != 0u) { if (dropped) *dropped += 1u; return list; }
    uint32_t i = 0;
    while (i < 4u && ((list >> (8u * i)) & 0xffu) != 0u && ((list >> (8u * i)) & 0xffu) <= id) ++i;
    const uint32_t low = list & ((1u << (8u * i)) - 1u), high = i == 3u ? 0u : (list >> (8u * i)) << (8u * (i + 1u));
    return low | id << (8u * i) | high;
}

// ---------------------------------------------------------------- light sampling (Hittable::sample / psa_pdf)
// rect.rs:113-173, sphere.rs:88-152, disk.rs:63-104, instance.rs:134-170; an emissive mesh face (the reference's todo!(), mesh.rs:213-232): DESIGN.md section 10.
// `entry`: the light-list entry that was picked (a mesh instance's entries name its emissive faces, PT_HDR_LIGHT_FACE_OFF).
PT_HD void light_sample(const SceneView& s, uint32_t inst, uint32_t entry, float sx, float sy, F3 from, F3* dir, float* pdf) {
    uint32_t kind = bu(s, inst + PT_INST_KIND), flags = bu(s, inst + PT_INST_FLAGS);
    bool xf = instance_is_transformed(s, inst), two_sided = (flags & 2u) != 0;
    if (xf) from = xf_point(s, inst + PT_INST_REVERSE, from);
    F3 origin = bf3(s, inst + PT_INST_ORIGIN);
    F3 point, normal; float area_pdf;
    if (kind == PT_SHAPE_RECT) {
        uint32_t axis = (flags >> 2) & 3u;
        float s0 = bf(s, inst + PT_INST_SIZE), s1 = bf(s, inst + PT_INST_SIZE + 1);
        float x = sx;
        normal = axis_vec(axis);
        if (two_sided) { float c = choose_first(&x, 0.5f) ? -1.0f : 1.0f; normal = mul(normal, c); }
        point = add(origin, rect_shuffle(f3((x - 0.5f) * s0, (sy - 0.5f) * s1, 0.0f), axis));
        area_pdf = 1.0f / (s0 * s1);
    } else if (kind == PT_SHAPE_SPHERE) {
        float radius = bf(s, inst + PT_INST_RADIUS);
        normal = random_on_unit_sphere(sx, sy);
        point = add(origin, mul(normal, radius));
        area_pdf = 1.0f / (radius * radius * 4.0f * PT_PI);
    } else if (!(s.lacks & PT_SCENE_NO_MESH_LIGHTS) && kind == PT_SHAPE_MESH) {
        // sample_surface of the face: the square-root mapping to barycentrics, the point and the normal hit_record reports there (the interpolated vertex
        // normal, or the face normal), no side choice, area pdf 1 / A_f (A_f computed once by the host); sample() on top of it as AARect's, below
        const uint32_t triw = bu(s, bu(s, PT_HDR_LIGHT_FACE_OFF) + entry);
        const uint32_t mesh = bu(s, inst + PT_INST_MESH), normal_off = bu(s, mesh + PT_MESH_NORMAL_OFF);
        const F4 q0 = mf4(s, triw), q1 = mf4(s, triw + 4), q2 = mf4(s, triw + 8);
        const float su = pt_sqrt(sx), b0 = 1.0f - su, b1 = sy * su, b2 = 1.0f - b0 - b1;
        point = add(add(mul(f3(q0.x, q0.y, q0.z), b0), mul(f3(q1.x, q1.y, q1.z), b1)), mul(f3(q2.x, q2.y, q2.z), b2));
        float area;
        if (normal_off != 0) {
            const uint32_t nn = normal_off + (triw - bu(s, mesh + PT_MESH_TRI_OFF));
            const F4 m0 = mf4(s, nn), m1 = mf4(s, nn + 4), m2 = mf4(s, nn + 8);
            normal = normalize(add(add(mul(f3(m0.x, m0.y, m0.z), b0), mul(f3(m1.x, m1.y, m1.z), b1)), mul(f3(m2.x, m2.y, m2.z), b2)));
            area = m0.w;
        } else {
            const F4 fn = mf4(s, pt_f2u(q1.w));
            normal = f3(fn.x, fn.y, fn.z);
            area = fn.w;
        }
        area_pdf = 1.0f / area;
    } else {
        float radius = bf(s, inst + PT_INST_RADIUS);
        float x = sx;
        normal = f3(0, 0, 1);
        if (two_sided) { float c = choose_first(&x, 0.5f) ? -1.0f : 1.0f; normal = mul(normal, c); }
        point = add(origin, mul(random_in_unit_disk(x, sy), radius));
        area_pdf = 1.0f / (PT_PI * radius * radius);
    }
    F3 direction = sub(point, from);
    float p;
    if (kind == PT_SHAPE_SPHERE) p = area_pdf * dot(direction, direction) / pt_abs(dot(normal, normalize(direction)));
    else { float cos_i = dot(normal, normalize(direction)); p = area_pdf * dot(direction, direction) / pt_abs(cos_i); }
    if (!pt_isfinite(p)) p = 0.0f;
    F3 dn = normalize(direction);
    if (xf) dn = normalize(xf_vec(s, inst + PT_INST_FORWARD, dn));
    *dir = dn; *pdf = p;
}
// `area`: for a hit on a mesh face, the A_f hit_record handed on in Hit::u (0: the hit is on no emissive face — its instance's own material emits — and the pdf is 0, as before)
PT_HD float light_psa_pdf(const SceneView& s, uint32_t inst, float cos_o, float cos_i, F3 from, F3 to, float area = 0.0f) {
    uint32_t kind = bu(s, inst + PT_INST_KIND);
    if (instance_is_transformed(s, inst)) { from = xf_point(s, inst + PT_INST_FORWARD, from); to = xf_point(s, inst + PT_INST_FORWARD, to); }
    F3 dd = sub(to, from);
    float d2 = dot(dd, dd);
    if (kind == PT_SHAPE_RECT) { float s0 = bf(s, inst + PT_INST_SIZE), s1 = bf(s, inst + PT_INST_SIZE + 1); return (1.0f / (s0 * s1)) * d2 / pt_abs(cos_i) / pt_abs(cos_o); }
    if (!(s.lacks & PT_SCENE_NO_MESH_LIGHTS) && kind == PT_SHAPE_MESH) return area > 0.0f ? (1.0f / area) * d2 / pt_abs(cos_i) / pt_abs(cos_o) : 0.0f;   // (the rect's form)
    float radius = bf(s, inst + PT_INST_RADIUS);
    if (kind == PT_SHAPE_SPHERE) return (1.0f / (radius * radius * 4.0f * PT_PI)) * d2 / pt_abs(cos_i * cos_o);
    if (kind == PT_SHAPE_DISK) return d2 / ((pt_abs(cos_o) * pt_abs(cos_i) + 0.00001f) * (PT_PI * radius * radius));
    return 0.0f;
}

// ---------------------------------------------------------------- environment (src/world/environment.rs)
// Curve::Linear{bounds (0,1), Nearest}.evaluate over a table in texture memory
// (`stride`: floats between consecutive entries — 2 where a pdf table is interleaved with its cmf, PT_HDR_IMAP_STRIDE)
PT_HD float linear01_nearest(const float* signal, uint32_t n, float x, uint32_t stride = 1u) {
    if (x < 0.0f || x > 1.0f) return 0.0f;
    float step = 1.0f / (float)n;
    float fi = x / step;
    uint32_t index = (uint32_t)fi;
    if (index >= n) index = n - 1;
    float left = signal[(size_t)index * stride];
    if (index + 1 >= n) return left;
    float t = (x - (float)index * step) / step;
    return t < 0.5f ? left : signal[(size_t)(index + 1) * stride];
}
// CurveWithCDF::sample_power_and_pdf on a (pdf, cmf) table pair (math crate, restated)
// `guide` (optional, n + 3 entries of u32 bits: entry j = lower bound of j / n) brackets the search: with
// j = max(0, floor(x n) - 1), j / n <= x < (j + 3) / n whatever the rounding, so the lower bound of x lies in
// [guide[j], guide[j + 3]] and the search inside the bracket returns the index the search of the whole table returns.
PT_HD void sample_cmf(const float* pdf, const float* cmf, uint32_t n, float x, float* coord, float* p, const float* guide = nullptr, uint32_t stride = 1u) {
    uint32_t lo = 0, hi = n;
    if (guide != nullptr && x >= 0.0f && x <= 1.0f) {
        float fj = pt_floor(x * (float)n) - 1.0f;
        uint32_t j = fj > 0.0f ? (uint32_t)fj : 0u;
        if (j > n - 1u) j = n - 1u;
        lo = pt_f2u(guide[j]); hi = pt_f2u(guide[j + 3u]);
    }
    while (lo < hi) { uint32_t mid = lo + (hi - lo) / 2; if (cmf[(size_t)mid * stride] < x) lo = mid + 1; else hi = mid; }
    uint32_t k = lo < n ? lo : n - 1;
    float below = k == 0 ? 0.0f : cmf[(size_t)(k - 1) * stride];
    float width = cmf[(size_t)k * stride] - below;
    float t = width > 0.0f ? (x - below) / width : 0.0f;
    float c = ((float)k + t) / (float)n;
    c = pt_clamp(c, 0.0f, 1.0f - PT_F32_EPSILON);
    *coord = c; *p = linear01_nearest(pdf, n, c, stride);
}
// What the emission and the pdf of an environment direction both start from, computed once per (u, v) (round 5: a vertex that left the scene took the direction of
// its (u, v) and — under an HDR map — that direction's texture coordinates twice, once for the pdf and once for the emission; a light sample took the direction once for
// its ray and again for its emission.  The same operations on the same values, made once: 2 sincos + atan2 + acos per environment vertex, 2 sincos per environment sample.)
struct EnvPoint { F3 dir; float u2, v2; };
PT_HD EnvPoint env_point_of(const SceneView& s, F3 dir) {   // dir = uv_to_direction(u, v)
    EnvPoint e; e.dir = dir; e.u2 = 0.0f; e.v2 = 0.0f;
    if (bu(s, PT_HDR_ENV_KIND) == PT_ENV_HDR) {
        // HDR (environment.rs:84-96): direction -> rotation.to_local -> equirect uv
        F3 nd = xf_vec(s, PT_HDR_ENV_REVERSE, dir);
        direction_to_uv(nd, &e.u2, &e.v2);
    }
    return e;
}
PT_HD EnvPoint env_point(const SceneView& s, float u, float v) {
    if (bu(s, PT_HDR_ENV_KIND) == PT_ENV_CONSTANT) { EnvPoint e; e.dir = f3(0, 0, 0); e.u2 = 0.0f; e.v2 = 0.0f; return e; }   // (nothing of it is read)
    return env_point_of(s, uv_to_direction(u, v));
}
PT_HD float env_emission(const SceneView& s, const EnvPoint& e, float lambda) {
    uint32_t kind = bu(s, PT_HDR_ENV_KIND);
    float strength = bf(s, PT_HDR_ENV_STRENGTH);
    if (kind == PT_ENV_CONSTANT) return curve_eval(s, bu(s, PT_HDR_ENV_CURVE), lambda) * strength;
    if (kind == PT_ENV_SUN) {
        F3 sd = bf3(s, PT_HDR_ENV_SUN_DIR);
        float c = dot(sd, e.dir), sn = pt_sqrt(1.0f - c * c);
        if (pt_abs(sn) < pt_sin(bf(s, PT_HDR_ENV_ANGULAR) / 2.0f) && c > 0.0f) return curve_eval(s, bu(s, PT_HDR_ENV_CURVE), lambda) * strength;
        return 0.0f;
    }
    return texstack_eval(s, bu(s, PT_HDR_ENV_TEXSTACK), lambda, e.u2, e.v2) * strength;   // -> TexStack
}
PT_HD float env_emission(const SceneView& s, float u, float v, float lambda) { return env_emission(s, env_point(s, u, v), lambda); }
// The same for the light samples of one vertex: an HDR environment of one layer (every HDRI of the reference's scene files)
// evaluates its curves once per vertex and wavelength instead of once per light sample.
struct EnvCurves { LayerCurves c; bool cached; };
PT_HD EnvCurves env_curves(const SceneView& s, float lambda) {
    EnvCurves e; e.cached = false; e.c.c0 = e.c.c1 = e.c.c2 = e.c.c3 = 0.0f;
    if (bu(s, PT_HDR_ENV_KIND) != PT_ENV_HDR) return e;
    const uint32_t ts = bu(s, PT_HDR_ENV_TEXSTACK);
    if (bu(s, ts) != 1u) return e;
    e.c = layer_curves(s, ts + 1, lambda); e.cached = true;
    return e;
}
PT_HD float env_emission(const SceneView& s, const EnvPoint& e, float lambda, const EnvCurves& ec) {
    if (!ec.cached) return env_emission(s, e, lambda);
    return (0.0f + layer_eval(s, bu(s, PT_HDR_ENV_TEXSTACK) + 1, ec.c, e.u2, e.v2)) * bf(s, PT_HDR_ENV_STRENGTH);
}
PT_HD float env_pdf_for(const SceneView& s, const EnvPoint& e) {
    uint32_t kind = bu(s, PT_HDR_ENV_KIND);
    if (kind == PT_ENV_SUN) {
        F3 sd = bf3(s, PT_HDR_ENV_SUN_DIR);
        float ad = bf(s, PT_HDR_ENV_ANGULAR);
        float c = dot(sd, e.dir), sn = pt_sqrt(1.0f - c * c);
        if (pt_abs(sn) < pt_sin(ad / 2.0f) && c > 0.0f) return 1.0f / (2.0f * PT_PI * (1.0f - pt_cos(ad)));
        return 0.0f;
    }
    uint32_t rows = bu(s, PT_HDR_IMAP_ROWS);
    if (kind == PT_ENV_HDR && rows > 0) {  // environment.rs:221-253
        uint32_t cols = bu(s, PT_HDR_IMAP_COLS);
        const float u2 = e.u2, v2 = e.v2;
        uint32_t row = (uint32_t)(pt_clamp(u2, 0.0f, 1.0f - PT_F32_EPSILON) * (float)rows);
#if defined(PT_EXP_TABLE_FOLD)
        row %= rows / PT_EXP_TABLE_FOLD;
#endif
        const uint32_t stride = bu(s, PT_HDR_IMAP_STRIDE);
        const float marginal_pdf = s.marg_words != 0u ? linear01_nearest(s.marg + (bu(s, PT_HDR_IMAP_MARG_PDF) - s.marg_base), rows, u2, stride)   // (the LDS copy: stage_marginal)
                                                       : linear01_nearest(s.tex + bu(s, PT_HDR_IMAP_MARG_PDF), rows, u2, stride);
        return marginal_pdf *
                   linear01_nearest(s.tex + bu(s, PT_HDR_IMAP_ROW_PDF) + (size_t)row * cols * stride, cols, v2, stride) *
                   (2.0f * PT_PI * PT_PI * pt_sin(PT_PI * v2) + 0.001f) +
               0.001f;
    }
    return 1.0f / (4.0f * PT_PI);
}
PT_HD float env_pdf_for(const SceneView& s, float u, float v) { return env_pdf_for(s, env_point(s, u, v)); }
PT_HD void env_sample_uv(const SceneView& s, float sx, float sy, float* u, float* v, float* pdf) {
    uint32_t kind = bu(s, PT_HDR_ENV_KIND);
    if (kind == PT_ENV_SUN) {
        float ad = bf(s, PT_HDR_ENV_ANGULAR);
        F3 local_wo = add(f3(0, 0, 1), mul(random_in_unit_disk(sx, sy), pt_sin(ad / 2.0f)));
        Frame fr = frame_from_normal(bf3(s, PT_HDR_ENV_SUN_DIR));
        F3 dir = to_world(fr, local_wo);
        direction_to_uv(normalize(dir), u, v);
        *pdf = 1.0f / (2.0f * PT_PI * (1.0f - pt_cos(ad)));
        return;
    }
    uint32_t rows = bu(s, PT_HDR_IMAP_ROWS);
    if (kind == PT_ENV_HDR && rows > 0) {  // environment.rs:331-350 + importance_map.rs:325-357
        uint32_t cols = bu(s, PT_HDR_IMAP_COLS);
        float mu, row_pdf, mv, column_pdf;
        const uint32_t mg = bu(s, PT_HDR_IMAP_MARG_GUIDE), rg = bu(s, PT_HDR_IMAP_ROW_GUIDE);
        const uint32_t stride = bu(s, PT_HDR_IMAP_STRIDE);
        // (two call sites, not one call on selected pointers: each keeps its address space — LDS reads here, global ones there)
        if (s.marg_words != 0u) sample_cmf(s.marg + (bu(s, PT_HDR_IMAP_MARG_PDF) - s.marg_base), s.marg + (bu(s, PT_HDR_IMAP_MARG_CMF) - s.marg_base), rows, sy, &mu, &row_pdf,
                                           s.marg_guide ? s.marg + s.marg_guide : nullptr, stride);
        else sample_cmf(s.tex + bu(s, PT_HDR_IMAP_MARG_PDF), s.tex + bu(s, PT_HDR_IMAP_MARG_CMF), rows, sy, &mu, &row_pdf, mg ? s.tex + mg : nullptr, stride);
        uint32_t row = (uint32_t)(mu * (float)rows);
#if defined(PT_EXP_TABLE_FOLD)
        // A TIMING experiment (round 6, profiles/r6_experiments.md; never the product — the results are wrong): the importance map's row tables and the environment's texels
        // folded onto 1 / PT_EXP_TABLE_FOLD of their rows.  The same instructions and the same number of reads from a working set that much smaller: what the FULL vertex form
        // would take if its table reads hit L2 — the ceiling of anything that reorders the searches (band passes) without removing them.
        row %= rows / PT_EXP_TABLE_FOLD;
#endif
        sample_cmf(s.tex + bu(s, PT_HDR_IMAP_ROW_PDF) + (size_t)row * cols * stride, s.tex + bu(s, PT_HDR_IMAP_ROW_CMF) + (size_t)row * cols * stride, cols, sx, &mv, &column_pdf,
                   rg ? s.tex + rg + (size_t)row * (cols + 3u) : nullptr, stride);
        F3 new_wo = xf_vec(s, PT_HDR_ENV_FORWARD, uv_to_direction(mu, mv));
        float u2, v2; direction_to_uv(new_wo, &u2, &v2);
        *u = u2; *v = v2;
        *pdf = row_pdf * column_pdf * (2.0f * PT_PI * PT_PI * pt_sin(PT_PI * v2) + 0.001f) + 0.001f;
        return;
    }
    *u = sx; *v = sy; *pdf = 1.0f / (4.0f * PT_PI);
}

// ---------------------------------------------------------------- camera (src/camera/projective_camera.rs:101-120)
struct CameraParams { F3 origin, u, v, lower_left, horizontal, vertical; float aperture_diameter; int kind; float span_x, span_y; F3 w; };

PT_HD void camera_ray(const CameraParams& c, uint64_t seed, uint32_t pixel, uint32_t sample, float fu, float fv, F3* o, F3* d) {
    if (c.kind == PT_CAMERA_PANORAMA) {
        // PanoramaCamera::get_ray (src/camera/panorama_camera.rs:71-95): azimuth from the centre line, elevation from the
        // horizon, no aperture and no sampler draw; the local vector goes to the world through the (u, v, w) frame
        float ax_ = c.span_x * (fu - 0.5f), ay_ = c.span_y * (0.5f - fv);
        float sx, cx, sy, cy;
        pt_sincos(ax_, &sx, &cx); pt_sincos(ay_, &sy, &cy);
        F3 l = f3(sx * cy, sy, cx * cy);
        *o = c.origin; *d = add(add(mul(c.u, l.x), mul(c.v, l.y)), mul(c.w, l.z));
        return;
    }
    float ax = 0.0f, ay = 0.0f;
    for (uint32_t blk = 0; blk < PT_APERTURE_BLOCKS; ++blk) {
        pt_f32x4 r = pt_draw4(seed, pixel, sample, PT_DIM_APERTURE0 + blk);
        float x = r.x * 2.0f - 1.0f, y = r.y * 2.0f - 1.0f;
        if (x * x + y * y <= 1.0f) { ax = x; ay = y; break; }
        x = r.z * 2.0f - 1.0f; y = r.w * 2.0f - 1.0f;
        if (x * x + y * y <= 1.0f) { ax = x; ay = y; break; }
    }
    F3 rd = mul(f3(ax, ay, 0.0f), c.aperture_diameter);
    F3 offset = add(mul(c.u, rd.x), mul(c.v, rd.y));
    F3 ro = add(c.origin, offset);
    F3 pop = add(add(c.lower_left, mul(c.horizontal, fu)), mul(c.vertical, fv));
    *o = ro; *d = normalize(sub(pop, ro));
}

// CIE fit (math::misc::{x_bar,y_bar,z_bar}), f64 as in the reference
PT_HD double gaussian64(double x, double alpha, double mu, double s1, double s2) {
    double t = (x - mu) / (x < mu ? s1 : s2);
    return alpha * pt_exp64(-(t * t) / 2.0);
}
PT_HD void xyz_bar_contract(float angstrom, float* xb, float* yb, float* zb) {
    double a = (double)angstrom;
    *xb = (float)(gaussian64(a, 1.056, 5998.0, 379.0, 310.0) + gaussian64(a, 0.362, 4420.0, 160.0, 267.0) + gaussian64(a, -0.065, 5011.0, 204.0, 262.0));
    *yb = (float)(gaussian64(a, 0.821, 5688.0, 469.0, 405.0) + gaussian64(a, 0.286, 5309.0, 163.0, 311.0));
    *zb = (float)(gaussian64(a, 1.217, 4370.0, 118.0, 360.0) + gaussian64(a, 0.681, 4590.0, 260.0, 138.0));
}
// The same three numbers at less than half the f64 instructions (round 5; k_accumulate is nothing but this function and a Philox draw per sample: 400 of the 690
// instructions of its loop were the seven Gaussians').  The function has ONE f32 argument and the wavelengths a render can draw lie in a narrow range, so the
// cheaper evaluation is not argued to be close enough — it is compared with the contract's over EVERY f32 in [PT_XYZ_FAST_LO, PT_XYZ_FAST_HI] (10 027 009 values
// x 3 outputs: tests/test_xyz_bar.py on the host build, tests/test_gpu_parity.py on the device against the oracle) and returns the same bits for each; outside
// the range the contract's form runs.  What differs inside: the division by the width and the halving folded into one constant (arg = d * d * (-0.5 / s^2)), no
// special cases in the exponential (-480 < arg <= 0 in the range), round-to-nearest-even for the power of two, the reduction and the Taylor polynomial as fused
// multiply-adds, degree 11 instead of 13, v_ldexp for the scaling.  Each of these moves a Gaussian by a few 1e-16 of its value; the f32 rounding of the sums
// does not see it anywhere in the range (a degree-9 polynomial, for comparison, changes 262 of the 30 million outputs).
#ifndef PT_XYZ_FAST
#define PT_XYZ_FAST 1
#endif
#define PT_XYZ_FAST_LO 3600.0f   /* angstrom; the reference's ranges are [3800, 7500] and [3700, 7900] (prelude.rs:23) */
#define PT_XYZ_FAST_HI 8000.0f
PT_HD double gaussian64_fast(double x, double mu, double s1, double s2) {
    const double d = x - mu;
    const double c = x < mu ? -0.5 / (s1 * s1) : -0.5 / (s2 * s2);
    const double arg = d * d * c;
    const double fk = __builtin_rint(arg * 1.4426950408889634074);
    double r = __builtin_fma(-fk, 6.93147180369123816490e-01, arg);
    r = __builtin_fma(-fk, 1.90821492927058770002e-10, r);
    double p = 1.0 / 39916800.0;
    p = __builtin_fma(p, r, 1.0 / 3628800.0);
    p = __builtin_fma(p, r, 1.0 / 362880.0);
    p = __builtin_fma(p, r, 1.0 / 40320.0);
    p = __builtin_fma(p, r, 1.0 / 5040.0);
    p = __builtin_fma(p, r, 1.0 / 720.0);
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)fk);
}
PT_HD void xyz_bar(float angstrom, float* xb, float* yb, float* zb) {
#if PT_XYZ_FAST
    if (angstrom >= PT_XYZ_FAST_LO && angstrom <= PT_XYZ_FAST_HI) {
        const double a = (double)angstrom;
        *xb = (float)(1.056 * gaussian64_fast(a, 5998.0, 379.0, 310.0) + 0.362 * gaussian64_fast(a, 4420.0, 160.0, 267.0) + -0.065 * gaussian64_fast(a, 5011.0, 204.0, 262.0));
        *yb = (float)(0.821 * gaussian64_fast(a, 5688.0, 469.0, 405.0) + 0.286 * gaussian64_fast(a, 5309.0, 163.0, 311.0));
        *zb = (float)(1.217 * gaussian64_fast(a, 4370.0, 118.0, 360.0) + 0.681 * gaussian64_fast(a, 4590.0, 260.0, 138.0));
        return;
    }
#endif
    xyz_bar_contract(angstrom, xb, yb, zb);
}

}  // namespace ptd
#endif
