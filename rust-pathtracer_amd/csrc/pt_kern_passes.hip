// pt_kern_passes.hip — the two kernel forms of a path-pass render (include/pt_light_groups.h) and their launchers: siblings of
// k_shade_groups and k_shadow_groups (pt_kern_groups.hip) — the FULL vertex form and the general light-sample form, one wavelength, unfused, no live list —
// that route every energy addition to the plane of its path class (pt_path_pass_rules.h) and carry the path state (d, k) from vertex to vertex in one word
// per slot.  A translation unit of its own: no other kernel family's device code knows of passes.
#include <cstdio>
#include <cstdlib>
#include "pt_kernels.h"
#include "pt_path_passes_launch.h"

namespace ptk {

// k_shade_groups' loop (pt_kern_groups.hip): the environment vertices of a wave's 64 items shaded at once, the surface vertices from the wave's list, 64 at a time.
// `state`: the pass's state plane, one word per slot (pp_state_words).
template <int USE_LDS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PT_SHADE_WAVES)))
k_shade_passes(const uint32_t* __restrict__ blob, uint32_t blob_words, const float* __restrict__ tex, RenderParams rp, uint32_t bounce, const uint32_t* __restrict__ pixels,
               Queue paths_in, Queue hits, Queue paths_out, Queue shadow, float* __restrict__ energy, uint32_t seg_cap, const uint32_t* __restrict__ count_in,
               uint32_t* __restrict__ count_out, uint32_t* __restrict__ shadow_count, unsigned long long* __restrict__ block_stats, uint32_t* __restrict__ state) {
    extern __shared__ __align__(16) uint32_t lds[];
    __shared__ uint32_t lds_counts[16];  // [0] path queue head, [1] item queue head, [4..6] statistics
    if (PT_EMPTY_SEGMENT_EXIT && count_in[blockIdx.x] == 0u) {
        if (threadIdx.x == 0) { count_out[blockIdx.x] = 0u; shadow_count[blockIdx.x] = 0u; shadow_count[gridDim.x + blockIdx.x] = 0u; }
        return;
    }
    if (threadIdx.x < 16) lds_counts[threadIdx.x] = 0;
    SceneView s = stage_scene<USE_LDS, 0u>(blob, blob_words, tex, lds);
    stage_marginal<USE_LDS>(s, blob, blob_words, lds);
    if (USE_LDS == PT_LDS_NONE) __syncthreads();
    const uint32_t base = blockIdx.x * seg_cap, n = count_in[blockIdx.x];
    uint32_t st_vertices = 0, st_shadow = 0, st_env = 0;
    const uint32_t rounds = (n + blockDim.x - 1) / blockDim.x;
    __shared__ uint32_t later[kBlock * 2];   // per wave: 128 item indices (fewer than 64 left over + at most 64 new)
    uint32_t* my_later = later + (threadIdx.x >> 6) * 128u;
    uint32_t later_count = 0;   // (wave-uniform)
    for (uint32_t r = 0;;) {  // whole waves stay in the loop: the appends are ballots
        uint32_t i = 0;
        bool active = false;
        if (later_count >= 64u || (r == rounds && later_count > 0u)) {
            const uint32_t take = later_count < 64u ? later_count : 64u;
            later_count -= take;
            active = lane_id() < take;
            if (active) i = my_later[later_count + lane_id()];
        } else if (r < rounds) {
            const uint32_t j = r * blockDim.x + threadIdx.x;
            ++r;
            active = j < n; i = base + j;
            const bool surface = active && qf(hits, HS_T, i) >= 0.0f;
            const unsigned long long m = __ballot(surface);
            if (surface) my_later[later_count + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull))] = i;
            later_count += (uint32_t)__popcll(m);
            active = active && !surface;
            __builtin_amdgcn_wave_barrier();   // (the list is the wave's own: its writes are in LDS before any of its lanes reads them)
        } else break;
        PathVertexT<1> pv; Hit hit; hit.valid = false;
        bool wants_item = false;
        if (active) {
            pv = load_path<1>(paths_in, i, bounce == 0u);
            hit = load_hit<false>(hits, i);
            pv.slot &= ~PT_PATH_INSIDE_MARK;
            wants_item = shade_wants_item(s, rp, hit);
        }
        const uint32_t ipos = base + shared_append(wants_item, &lds_counts[1]);
        ShadeOutT<1> out;
        out.survives = false; out.has_item = false; out.vertex_pushed = false; out.env_hit = false; out.shadow_count = 0; out.add_energy = false; out.env_mask = 0;
        if (active) {
            const uint32_t pixel = pixels[pv.slot % rp.chunk_pixels];
            // the state in front of this vertex (the camera vertex: d = 0, nothing read), the kind of its material, and the item word the ray sink fills
            const uint32_t before = bounce == 0u ? 0u : state[pv.slot];
            const uint32_t d = pp_state_d(before), k = pp_state_k(before);
            const bool diffuse = hit.valid ? pp_kind_is_diffuse(bu(s, material_record(s, hit.material) + PT_MAT_KIND)) : true;
            uint32_t word = pp_item_classes(d, k, diffuse);
            out = stage_shade<1, true, true>(s, rp, bounce, pv, hit, pixel, [&](uint32_t l, const ShadowRayT<1>& ray) {
                store_shadow_ray<1>(shadow, ipos, l, ray);
                word |= pp_item_ray_bit(d, diffuse, hit.n, pv.d, l, ray.d);
            });
            if (wants_item) {
                qsu(shadow, Layout<1>::sh_slot, ipos, pv.slot); qsu(shadow, Layout<1>::sh_flags, ipos, out.env_mask);
                qsf(shadow, Layout<1>::sh_lambda, ipos, pv.lambda);
                if (!out.has_item) clear_shadow_item<1>(shadow, ipos, rp.light_samples);
            }
            if (out.add_energy) {
                energy[pv.slot] += out.energy_add[0];
                pp_add_vertex(d, k, hit.valid, out.energy_add[0], energy, rp.energy_stride, pv.slot);
            }
            if (hit.valid) state[pv.slot] = word | (out.survives ? pp_next_state(d, k, pp_event_kind(diffuse, hit.n, pv.d, out.next.d)) : 0u);
        }
        const uint32_t pos = base + shared_append(out.survives, &lds_counts[0]);
        if (out.survives) store_path<1>(paths_out, pos, out.next);
        st_vertices += out.vertex_pushed ? 1u : 0u; st_env += out.env_hit ? 1u : 0u; st_shadow += out.shadow_count;
    }
    st_vertices = wave_reduce_add(st_vertices); st_shadow = wave_reduce_add(st_shadow); st_env = wave_reduce_add(st_env);
    if (lane_id() == 0) { atomicAdd(&lds_counts[4], st_vertices); atomicAdd(&lds_counts[5], st_shadow); atomicAdd(&lds_counts[6], st_env); }
    __syncthreads();
    if (threadIdx.x == 0) {
        count_out[blockIdx.x] = lds_counts[0]; shadow_count[blockIdx.x] = lds_counts[1]; shadow_count[gridDim.x + blockIdx.x] = 0u;
        unsigned long long* bs = block_stats + (size_t)blockIdx.x * BS_FIELDS;
        bs[BS_VERTICES] += lds_counts[4]; bs[BS_SHADOW_RAYS] += lds_counts[5]; bs[BS_ENV_HITS] += lds_counts[6];
        bs[BS_SEGMENTS] += n;
        bs[BS_ITEMS] += lds_counts[1];
    }
}

// k_shadow's general form (pt_kernels.h): every item of the segment, no list of live ones
template <int USE_LDS>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PT_WALK_WAVES)))
k_shadow_passes(const uint32_t* __restrict__ blob, uint32_t blob_words, const float* __restrict__ tex, uint32_t light_samples, Queue shadow, float* __restrict__ energy,
                uint32_t energy_stride, uint32_t seg_cap, const uint32_t* __restrict__ count_in, const uint32_t* __restrict__ state) {
    extern __shared__ __align__(16) uint32_t lds[];
    if (PT_EMPTY_SEGMENT_EXIT && count_in[blockIdx.x] == 0u) return;
    SceneView s = stage_scene<USE_LDS, 0u>(blob, blob_words, tex, lds);
    const uint32_t base = blockIdx.x * seg_cap, n = count_in[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) pp_shadow_item<PT_TRAV_ANY>(s, light_samples, shadow, base + j, energy, energy_stride, state);
}

#define PT_PASSES_BY_MODE(cfg, K, ...) do { if (c.lds_mode == PT_LDS_ALL) go(cfg, K<PT_LDS_ALL>, __VA_ARGS__); else if (c.lds_mode == PT_LDS_CORE) go(cfg, K<PT_LDS_CORE>, __VA_ARGS__); \
                                            else go(cfg, K<PT_LDS_NONE>, __VA_ARGS__); } while (0)

void launch_shade_passes(const LaunchCfg& c, const SceneArgs& sc, const RenderParams& rp, uint32_t bounce, const uint32_t* pixels, Queue paths_in, Queue hits, Queue paths_out,
                         Queue shadow, float* energy, uint32_t seg_cap, const uint32_t* count_in, uint32_t* count_out, uint32_t* shadow_count, unsigned long long* block_stats) {
    if (rp.camera_record == 0u || rp.live_list != 0u) { fprintf(stderr, "launch_shade_passes: the FULL form reads the camera vertex' lean record and builds no live list\n"); abort(); }
    LaunchCfg d = c; d.lds_bytes = ((c.lds_bytes + 15u) & ~15u) + sc.marg_bytes;   // (the marginal tables of the importance map behind the blob: stage_marginal)
    PT_PASSES_BY_MODE(d, k_shade_passes, sc.blob, sc.blob_words, sc.tex, rp, bounce, pixels, paths_in, hits, paths_out, shadow, energy, seg_cap, count_in, count_out, shadow_count,
                      block_stats, pp_state_words(energy, rp.energy_stride));
}

void launch_shadow_passes(const LaunchCfg& c, const SceneArgs& sc, uint32_t light_samples, Queue shadow, float* energy, uint32_t energy_stride, uint32_t seg_cap,
                          const uint32_t* count_in) {
    PT_PASSES_BY_MODE(c, k_shadow_passes, sc.blob, sc.blob_words, sc.tex, light_samples, shadow, energy, energy_stride, seg_cap, count_in,
                      (const uint32_t*)pp_state_words(energy, energy_stride));
}

hipError_t allow_lds_passes(uint32_t shade_bytes, uint32_t shadow_bytes) {
    hipError_t worst = hipSuccess;
    auto allow = [&](const void* k, uint32_t bytes) { hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); if (e != hipSuccess) worst = e; };
    allow(reinterpret_cast<const void*>(k_shade_passes<PT_LDS_ALL>), shade_bytes); allow(reinterpret_cast<const void*>(k_shade_passes<PT_LDS_CORE>), shade_bytes);
    allow(reinterpret_cast<const void*>(k_shadow_passes<PT_LDS_ALL>), shadow_bytes); allow(reinterpret_cast<const void*>(k_shadow_passes<PT_LDS_CORE>), shadow_bytes);
    return worst;
}

}  // namespace ptk
