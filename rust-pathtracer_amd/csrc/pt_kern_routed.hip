// pt_kern_routed.hip — the two kernel forms of a routed render and their launchers: siblings of k_shade<M, 1, PT_SHADE_FULL, 0u> and
// k_shadow<M, 1, PT_TRAV_ANY, true, 0u> — the most general vertex and light-sample forms, one wavelength, unfused, no live list — that also send every energy
// addition to the plane their router names (pt_routed_rules.h): the light group's for a light-group render (include/pt_light_groups.h),
// the path class's for a path-pass render (section 17), every matching expression's for a path-expression render (section 17).  A translation unit of its own: no other kernel family's device code knows of routers.
#include <cstdio>
#include <cstdlib>
#include "pt_kernels.h"
#include "pt_routed_launch.h"

namespace ptk {

// A router crosses the launch as its Arg (pt_routed_rules.h): a kernel argument of its own can be __restrict__, a struct's member cannot.

// k_shade's FULL form (pt_kernels.h): the environment vertices of a wave's 64 items shaded at once, the surface vertices from the wave's list, 64 at a time.
template <int USE_LDS, typename Router>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PT_SHADE_WAVES)))
k_shade_routed(const uint32_t* __restrict__ blob, uint32_t blob_words, const float* __restrict__ tex, RenderParams rp, uint32_t bounce, const uint32_t* __restrict__ pixels,
               Queue paths_in, Queue hits, Queue paths_out, Queue shadow, float* __restrict__ energy, uint32_t seg_cap, const uint32_t* __restrict__ count_in,
               uint32_t* __restrict__ count_out, uint32_t* __restrict__ shadow_count, unsigned long long* __restrict__ block_stats, typename Router::Arg router_arg) {
    const Router router{router_arg};
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
        if (active)
            out = routed_vertex(s, rp, router, bounce, pv, hit, pixels[pv.slot % rp.chunk_pixels], wants_item, shadow, ipos, energy, [](const typename Router::Vertex&, const Hit&) {});
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
template <int USE_LDS, typename Router>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PT_WALK_WAVES)))
k_shadow_routed(const uint32_t* __restrict__ blob, uint32_t blob_words, const float* __restrict__ tex, uint32_t light_samples, Queue shadow, float* __restrict__ energy,
                uint32_t energy_stride, uint32_t seg_cap, const uint32_t* __restrict__ count_in, typename Router::Arg router_arg) {
    const Router router{router_arg};
    extern __shared__ __align__(16) uint32_t lds[];
    if (PT_EMPTY_SEGMENT_EXIT && count_in[blockIdx.x] == 0u) return;
    SceneView s = stage_scene<USE_LDS, 0u>(blob, blob_words, tex, lds);
    const uint32_t base = blockIdx.x * seg_cap, n = count_in[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) routed_shadow_item<PT_TRAV_ANY>(s, router, light_samples, shadow, base + j, energy, energy_stride);
}

// the kernel of the launch's staging mode (PT_LDS_*) among a form's three
template <typename K, typename... Args>
static void go_by_mode(const LaunchCfg& cfg, K all, K core, K none, Args... args) {
    go(cfg, cfg.lds_mode == PT_LDS_ALL ? all : cfg.lds_mode == PT_LDS_CORE ? core : none, args...);
}

template <typename Router>
void launch_shade_routed(const LaunchCfg& c, const SceneArgs& sc, const RenderParams& rp, uint32_t bounce, const uint32_t* pixels, Queue paths_in, Queue hits, Queue paths_out,
                         Queue shadow, float* energy, uint32_t seg_cap, const uint32_t* count_in, uint32_t* count_out, uint32_t* shadow_count, unsigned long long* block_stats,
                         const Router& router) {
    if (rp.camera_record == 0u || rp.live_list != 0u) { fprintf(stderr, "launch_shade_routed: the FULL form reads the camera vertex' lean record and builds no live list\n"); abort(); }
    LaunchCfg d = c; d.lds_bytes = ((c.lds_bytes + 15u) & ~15u) + sc.marg_bytes;   // (the marginal tables of the importance map behind the blob: stage_marginal)
    go_by_mode(d, k_shade_routed<PT_LDS_ALL, Router>, k_shade_routed<PT_LDS_CORE, Router>, k_shade_routed<PT_LDS_NONE, Router>, sc.blob, sc.blob_words, sc.tex, rp, bounce, pixels,
               paths_in, hits, paths_out, shadow, energy, seg_cap, count_in, count_out, shadow_count, block_stats, router.arg());
}

template <typename Router>
void launch_shadow_routed(const LaunchCfg& c, const SceneArgs& sc, uint32_t light_samples, Queue shadow, float* energy, uint32_t energy_stride, uint32_t seg_cap,
                          const uint32_t* count_in, const Router& router) {
    go_by_mode(c, k_shadow_routed<PT_LDS_ALL, Router>, k_shadow_routed<PT_LDS_CORE, Router>, k_shadow_routed<PT_LDS_NONE, Router>, sc.blob, sc.blob_words, sc.tex, light_samples,
               shadow, energy, energy_stride, seg_cap, count_in, router.arg());
}

#define PT_ROUTED_LAUNCHERS(Router) \
    template void launch_shade_routed<Router>(const LaunchCfg&, const SceneArgs&, const RenderParams&, uint32_t, const uint32_t*, Queue, Queue, Queue, Queue, float*, uint32_t, \
                                              const uint32_t*, uint32_t*, uint32_t*, unsigned long long*, const Router&); \
    template void launch_shadow_routed<Router>(const LaunchCfg&, const SceneArgs&, uint32_t, Queue, float*, uint32_t, uint32_t, const uint32_t*, const Router&);
PT_ROUTED_LAUNCHERS(GroupRouter)
PT_ROUTED_LAUNCHERS(PassRouter)
PT_ROUTED_LAUNCHERS(ExprRouter)

template <typename Router>
static void allow_lds_router(uint32_t shade_bytes, uint32_t shadow_bytes, hipError_t* worst) {
    auto allow = [&](const void* k, uint32_t bytes) { hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); if (e != hipSuccess) *worst = e; };
    allow(reinterpret_cast<const void*>(k_shade_routed<PT_LDS_ALL, Router>), shade_bytes); allow(reinterpret_cast<const void*>(k_shade_routed<PT_LDS_CORE, Router>), shade_bytes);
    allow(reinterpret_cast<const void*>(k_shadow_routed<PT_LDS_ALL, Router>), shadow_bytes); allow(reinterpret_cast<const void*>(k_shadow_routed<PT_LDS_CORE, Router>), shadow_bytes);
}

hipError_t allow_lds_routed(uint32_t shade_bytes, uint32_t shadow_bytes) {
    hipError_t worst = hipSuccess;
    allow_lds_router<GroupRouter>(shade_bytes, shadow_bytes, &worst);
    allow_lds_router<PassRouter>(shade_bytes, shadow_bytes, &worst);
    allow_lds_router<ExprRouter>(shade_bytes, shadow_bytes, &worst);
    return worst;
}

}  // namespace ptk
