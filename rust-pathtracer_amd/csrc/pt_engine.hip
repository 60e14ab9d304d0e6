// pt_engine.hip — the host side of the HIP engine behind include/pt_api.h (gfx950 / MI355X only).
//
// Scene upload (one flat blob + texels per device), buffer management, the pass loop — per bounce one launch each of extend -> shade ->
// shadow over segmented SoA queues in HBM, with HIP events around every launch so that per-stage device time is measured inside the
// timed region —, the choice of kernel variant per scene (pt_launch.h: staging mode x traversal form x wavelengths x what the scene can
// need), the probes of the trait surface, and pt_render_multi: one replica, host thread and stream per device and one RCCL reduce.
// Around a film: the probe pass (probe_params, launch_probe) behind pt_camera_samples, pt_intersect, the one guide pass (render_guides_impl: the first
// hit's loop or the chain's) and the ID mattes; apply_resident, the one "parameter block up, launch over resident planes, output back" behind the resident
// mix, develop, re-lamp and extract entries and each device of run_resident_shards; and the resident filters' shared reserve, fill and run.
// The kernels themselves are templates in pt_kernels.h, instantiated per family in pt_kern_*.hip.  No CPU fallback: every entry point
// fails with PT_ERR_NO_DEVICE when HIP has no device.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_kernels.h"   /* first: it switches on the wave-level device code of pt_device.h */
#include "../../include/pt_adaptive.h"
#include "../../include/pt_spectral.h"
#include "../../include/pt_api.h"
#include "../../include/pt_debug.h"
#include "../../include/pt_denoise.h"
#include "../../include/pt_light_groups.h"
#include "../../include/pt_light_groups_denoise.h"
#include "../../include/pt_light_groups_multi.h"
#include "../../include/pt_light_groups_spectral.h"
#include "pt_adaptive_select.h"
#include "pt_light_groups_launch.h"
#include "pt_routed_launch.h"
#include "pt_light_groups_spectral_launch.h"
#include "pt_spectral_launch.h"
#include "pt_spectral_rules.h"
#include "pt_spectral_project_launch.h"
#include "pt_shard_launch.h"
#include "pt_shard_rules.h"
#include "pt_denoise_launch.h"
#include "pt_denoise_resident_launch.h"
#include "pt_error.h"
#include "pt_guides_chain_launch.h"
#include "pt_matte_launch.h"
#include "pt_matte_rules.h"
#include "pt_denoise_spectral_albedo_launch.h"
#include "pt_plan.h"
#include "pt_scene_host.h"

using namespace ptd;
using namespace ptk;

namespace {

thread_local std::string g_error;
pt_status fail(pt_status st, const std::string& msg) { g_error = msg; return st; }
}  // namespace
void pt_set_error(const std::string& message) { g_error = message; }
namespace {

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : (e_ == hipErrorNoDevice ? PT_ERR_NO_DEVICE : PT_ERR_DEVICE), \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                                    \
    } while (0)

// mode 0: generate_and_evaluate(lambda, wi, s2) -> f, wo, pdf ; 1: bsdf(lambda, wi, wo) -> f, pdf ; 2: emission(lambda, wi) ; 3: curve(lambda)
// the first stage of a camera sample as k_generate runs it (stage_generate), for chosen (pixel, sample) pairs: pt_camera_samples
__global__ void __launch_bounds__(kBlock) k_probe_camera(RenderParams rp, uint32_t n, const uint32_t* __restrict__ pixel, const uint32_t* __restrict__ sample,
                                                        float* __restrict__ o, float* __restrict__ d, float* __restrict__ lambda) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const PathVertexT<1> p = stage_generate<1>(rp, sample[i], pixel[i]);
        o[3 * i] = p.o.x; o[3 * i + 1] = p.o.y; o[3 * i + 2] = p.o.z;
        d[3 * i] = p.d.x; d[3 * i + 1] = p.d.y; d[3 * i + 2] = p.d.z;
        lambda[i] = p.lambda;
    }
}
__global__ void __launch_bounds__(kBlock) k_probe_material(const uint32_t* __restrict__ blob, const float* __restrict__ tex, int mode, uint32_t record, uint32_t n,
                                                          const float* __restrict__ lambda, const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ f, float* __restrict__ wo, float* __restrict__ pdf) {
    SceneView s; s.w = blob; s.tex = tex; s.m = blob + blob[PT_HDR_CORE_WORDS];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (mode == 0) {
            F3 w; material_sample(s, record, lambda[i], 0.5f, 0.5f, b[2 * i], b[2 * i + 1], f3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), &f[i], &w, &pdf[i]);
            wo[3 * i] = w.x; wo[3 * i + 1] = w.y; wo[3 * i + 2] = w.z;
        } else if (mode == 1) {
            material_bsdf(s, record, lambda[i], 0.5f, 0.5f, f3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), f3(b[3 * i], b[3 * i + 1], b[3 * i + 2]), &f[i], &pdf[i]);
        } else if (mode == 2) {
            f[i] = material_emission(s, record, lambda[i], f3(a[3 * i], a[3 * i + 1], a[3 * i + 2]));
        } else {
            f[i] = curve_eval(s, record, lambda[i]);
        }
    }
}
// light_sample of one light-list entry from n points (pt_light_sample): the vertex kernels' own call, every shape's code present (lacks = 0)
__global__ void __launch_bounds__(kBlock) k_probe_light(const uint32_t* __restrict__ blob, const float* __restrict__ tex, uint32_t entry, uint32_t n,
                                                       const float* __restrict__ from, const float* __restrict__ s2, float* __restrict__ dir, float* __restrict__ pdf) {
    SceneView s; s.w = blob; s.tex = tex; s.m = blob + blob[PT_HDR_CORE_WORDS];
    const uint32_t inst = blob[PT_HDR_INSTANCE_OFF] + blob[blob[PT_HDR_LIGHT_OFF] + entry] * PT_INST_WORDS;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        F3 d;
        light_sample(s, inst, entry, s2[2 * i], s2[2 * i + 1], f3(from[3 * i], from[3 * i + 1], from[3 * i + 2]), &d, &pdf[i]);
        dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
    }
}
__global__ void __launch_bounds__(kBlock) k_probe_numerics(int which, uint32_t n, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float r;
        switch (which) {
            case 0: r = pt_sin(x[i]); break;
            case 1: r = pt_cos(x[i]); break;
            case 2: r = pt_exp(x[i]); break;
            case 3: r = pt_pow(x[i], y[i]); break;
            case 4: r = pt_acos(x[i]); break;
            case 5: r = pt_atan2(x[i], y[i]); break;
            case 6: r = (float)pt_exp64((double)x[i]); break;
            case 7: r = (float)pt_log64((double)x[i]); break;
            case 8: r = x[i] / y[i]; break;
            case 9: r = pt_sqrt(x[i]); break;
            case 10: r = x[i] * y[i] + x[i]; break;  // must NOT be contracted to an fma
            case 11: case 12: case 13: { float c[3]; ptd::xyz_bar(x[i], &c[0], &c[1], &c[2]); r = c[which - 11]; break; }   // x = angstrom
            default: r = 0.0f;
        }
        out[i] = r;
    }
}

// ---- adaptive sampling (include/pt_adaptive.h): one round's decision and the stable compaction of the next pixel list.
// mark: every pixel of the round's list takes the list's count and its decision (the byte image was cleared before the launch, so it marks exactly
// the pixels of this list that are not converged)
__global__ void __launch_bounds__(kBlock) k_adaptive_mark(const uint32_t* __restrict__ list, uint32_t n, uint32_t count, const double* __restrict__ stats,
                                                         float rel_error, float abs_error, uint32_t* __restrict__ counts, uint8_t* __restrict__ unconverged) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t p = list[i];
        counts[p] = count;
        unconverged[p] = adaptive_unconverged(count, stats[2 * (size_t)p], stats[2 * (size_t)p + 1], rel_error, abs_error) ? 1u : 0u;
    }
}
// keep: one list entry per thread; workgroup b writes how many of its kBlock entries stay (wave ballots), block_counts[b]
__global__ void __launch_bounds__(kBlock) k_adaptive_keep(const uint32_t* __restrict__ list, uint32_t n, uint32_t count, uint32_t max_samples,
                                                         const uint8_t* __restrict__ unconverged, uint32_t width, uint32_t height, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t wave_kept[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = i < n && adaptive_keep(unconverged, width, height, list[i], count, max_samples);
    const unsigned long long m = __ballot(keep);
    if (lane_id() == 0) wave_kept[threadIdx.x / 64] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t kept = 0;
        for (int w = 0; w < kBlock / 64; ++w) kept += wave_kept[w];
        block_counts[blockIdx.x] = kept;
    }
}
// scan: one workgroup turns the nb block counts into exclusive offsets in place and writes the total behind them (block_counts[nb])
__global__ void __launch_bounds__(kBlock) k_adaptive_scan(uint32_t* __restrict__ block_counts, uint32_t nb) {
    __shared__ uint32_t sum[kBlock];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? block_counts[i] : 0u;
        sum[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1; d < (uint32_t)kBlock; d <<= 1) {   // (inclusive Hillis-Steele scan of the chunk)
            const uint32_t t = threadIdx.x >= d ? sum[threadIdx.x - d] : 0u;
            __syncthreads();
            sum[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb) block_counts[i] = carry + sum[threadIdx.x] - v;
        carry += sum[kBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_counts[nb] = carry;
}
// scatter: the kept entries in list order — workgroup offset, then the waves before this one, then the lanes below this one
__global__ void __launch_bounds__(kBlock) k_adaptive_scatter(const uint32_t* __restrict__ list, uint32_t n, uint32_t count, uint32_t max_samples,
                                                            const uint8_t* __restrict__ unconverged, uint32_t width, uint32_t height,
                                                            const uint32_t* __restrict__ offsets, uint32_t* __restrict__ next) {
    __shared__ uint32_t wave_kept[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = i < n && adaptive_keep(unconverged, width, height, list[i], count, max_samples);
    const unsigned long long m = __ballot(keep);
    if (lane_id() == 0) wave_kept[threadIdx.x / 64] = (uint32_t)__popcll(m);
    __syncthreads();
    if (keep) {
        uint32_t o = offsets[blockIdx.x];
        for (uint32_t w = 0; w < threadIdx.x / 64; ++w) o += wave_kept[w];
        next[o + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull))] = list[i];
    }
}
// finish: every pixel of the film divided by its own count (pt_render's division by spp, stage_accumulate_pixel), W = 0.  A pixel of count 0 is
// another device's (pt_render_adaptive_multi) and stays 0: the node's gather adds the films.  On one device every count is at least spp.
__global__ void __launch_bounds__(kBlock) k_adaptive_finish(uint32_t n_pixels, const uint32_t* __restrict__ counts, float* __restrict__ film) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += gridDim.x * blockDim.x) {
        const uint32_t n = counts[p];
        if (n == 0u) continue;
        float4* px = reinterpret_cast<float4*>(film) + p;
        const float4 v = *px;
        const float c = (float)n;
        *px = make_float4(v.x / c, v.y / c, v.z / c, 0.0f);
    }
}
// finish of pt_render_adaptive_spectral: every bin of a pixel divided by the pixel's own count (spectral_finish_value); plane by plane, so that neighbouring
// lanes touch neighbouring floats
__global__ void __launch_bounds__(kBlock) k_adaptive_finish_spectral(uint32_t n_pixels, uint32_t bins, const uint32_t* __restrict__ counts, float* __restrict__ spectral) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += gridDim.x * blockDim.x) {
        const uint32_t n = counts[p];
        float* px = spectral + p;
        for (uint32_t b = 0; b < bins; ++b) px[(size_t)b * n_pixels] = spectral_finish_value(px[(size_t)b * n_pixels], n);
    }
}
// the exchange of pt_render_adaptive_multi between the virtual devices of one physical device: dst |= src over two unconverged images of n bytes
// (0 / 1 per pixel; each device marks only its own shard's pixels, so the OR is the film-wide image), 16 bytes per lane and the tail byte by byte
__global__ void __launch_bounds__(kBlock) k_mask_or(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t n) {
    const size_t n16 = n / 16, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4* d = reinterpret_cast<uint4*>(dst);
    const uint4* s = reinterpret_cast<const uint4*>(src);
    for (size_t i = first; i < n16; i += stride) {
        const uint4 a = d[i], b = s[i];
        d[i] = make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w);
    }
    for (size_t i = n16 * 16 + first; i < n; i += stride) dst[i] = (uint8_t)(dst[i] | src[i]);
}

// ------------------------------------------------------------------------------------------------ host side
// A device allocation (pinned: a page-locked host one) that is freed on every way out of its scope (the probes below return early on any HIP error).
struct DevBuf {
    void* p = nullptr;
    bool pinned = false;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p && pinned) hipHostFree(p); else if (p) hipFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};
// One that only grows: its owner keeps it between calls, so that a sequence of renders allocates it once; a call that needs more replaces it, and it is freed
// with its owner.
struct GrowBuf : DevBuf {
    size_t bytes = 0;
    pt_status reserve(size_t want) {
        if (bytes >= want) return PT_OK;
        release();
        bytes = 0;
        if (pinned) HIP_TRY(hipHostMalloc(&p, want, hipHostMallocPortable));
        else HIP_TRY(hipMalloc(&p, want));
        bytes = want;
        return PT_OK;
    }
};

constexpr uint32_t kUnitCounters = 2 * 64 + 2;   // two parked launches per bounce, max_bounces <= 64
struct DeviceBuffers {
    uint32_t capacity = 0, light_samples = 0, nl = 0, park_block = 0;
    uint32_t energy_planes = 0;   // planes of `energy`: nl + 1, or a light-group render's 2 + G (pt_light_group_rules.h)
    uint32_t *paths_a = nullptr, *paths_b = nullptr, *hits = nullptr, *shadow = nullptr, *pixels = nullptr, *counts = nullptr, *park = nullptr;
    uint32_t* unit_counters = nullptr;   // parked kernels with dynamic units: one counter per launch of a pass (kUnitCounters), zeroed per pass
    float* energy = nullptr;
    unsigned long long* block_stats = nullptr;
    size_t pixel_capacity = 0;
    int grid = 0;  // segments per queue == workgroups per launch
    void release() {
        hipFree(paths_a); hipFree(paths_b); hipFree(hits); hipFree(shadow); hipFree(pixels); hipFree(counts); hipFree(energy); hipFree(block_stats); hipFree(park);
        hipFree(unit_counters);
        *this = DeviceBuffers();
    }
};
// pt_render_adaptive: per film pixel its count, (S1, S2) and the unconverged byte; the round's pixel list and the next; the keep kernel's per-workgroup
// counts, scanned in place, with the total behind them
struct AdaptiveBuffers {
    size_t pixels = 0;
    uint32_t *counts = nullptr, *lists[2] = {nullptr, nullptr}, *block_counts = nullptr;
    double* stats = nullptr;
    uint8_t* unconverged = nullptr;
    void release() {
        hipFree(counts); hipFree(lists[0]); hipFree(lists[1]); hipFree(block_counts); hipFree(stats); hipFree(unconverged);
        *this = AdaptiveBuffers();
    }
};

}  // namespace

// What the last adaptive node render (render_node) left where, for pt_resident_assemble (include/pt_resident.h): film, counts and statistics on `device`, the
// first device of the mask and, per kind of packed shard (a spectral render's bins in spectral_shard, a group render's films in group_shard), the scenes that hold
// the shards and their number of planes.  Kept with the MultiSetup whose films it points into: released with it.  Every render entry forgets it when it starts.
struct NodeRemembered {
    pth::NodeRender info;
    int device = 0;
    const float* film = nullptr; const uint32_t* counts = nullptr; const double* stats = nullptr;
    struct Shards { std::vector<pt_scene*> scenes; uint32_t planes = 0; };
    Shards spectral, groups;
};

// What pt_render_multi sets up for a set of devices and a film size, kept on the scene: a frame-by-frame caller pays for streams, device
// films and the RCCL communicator once (round-2 advice: they were made and destroyed on every call, outside the timed window).
struct MultiSetup {
    std::vector<int> devices;         // physical devices of the mask
    uint32_t virt = 1;                // virtual devices per physical one (pt_tuning::multi_virtual)
    bool rccl = false;
    size_t film_bytes = 0;
    std::vector<float*> films;        // per virtual device, on its physical device
    std::vector<hipStream_t> streams; // per virtual device
    std::vector<ncclComm_t> comms;    // per physical device (rccl only)
    std::vector<GrowBuf> staging;   // per virtual device: the pinned host buffer its packed shard lands in (NodePayload: the spectral and the group node entries; grown on demand)
    NodeRemembered node_render;
    bool valid = false;
};

// include/pt_resident.h: what the scene holds on its device for pt_denoise_resident.  film, counts, stats and spectral point into the buffers of the render that
// made them resident (film_cache, the adaptive buffers, spectral_cache) or into load_*, pt_resident_load's own: that entry never writes a render's buffer, so
// spectral_valid keeps its meaning.  Everything else lies in buffers that only grow, so a repeated call allocates nothing.
struct ResidentSet {
    uint32_t parts = 0, width = 0, height = 0, bins = 0;   // PT_RESIDENT_* bits; bins: of the bins, the per-bin albedo and the denoised bins
    const float* film = nullptr; const uint32_t* counts = nullptr; const double* stats = nullptr; const float* spectral = nullptr;
    const float* denoised_bins = nullptr;   // in den_bins (the quad form) or in a bin_buf (the planar form)
    GrowBuf load_film, load_counts, load_stats, load_spectral;
    GrowBuf guides, albedo, bin_albedo;
    GrowBuf color[2], geo, tent, flags, grad, bin_buf[2];   // the filter's scratch (ptk::DnRun)
    GrowBuf den_film, den_var, den_bins;
    void end() { parts = 0; width = height = bins = 0; }
    void tidy() {
        if (!(parts & (PT_RESIDENT_BINS | PT_RESIDENT_BIN_ALBEDO | PT_RESIDENT_DENOISED_BINS))) bins = 0;
        if (!parts) width = height = 0;
    }
    struct pt_resident_info info() const { struct pt_resident_info i; i.width = width; i.height = height; i.bins = bins; i.parts = parts; return i; }
};

// A scene's shard of a node render, kept on it (pt_shard_rules.h): px, the pixel list in pth::shard_pixels' order, and packed, the planes of px.size() elements
// on its device that the pack kernel left (k_spectral_pack: floats; k_light_groups_pack: float4).
struct Shard {
    std::vector<uint32_t> px;
    GrowBuf packed;
};

struct pt_scene {
    pth::HostScene host;
    pt_tuning tuning;
    MultiSetup multi;
    uint32_t* d_blob = nullptr;
    float* d_tex = nullptr;
    uint32_t blob_words = 0;
    int lds_mode = 0;  // PT_LDS_*
    uint32_t lacks = 0; // PT_SCENE_* bits: what the scene does not hold (kernel forms without it)
    int device = 0, num_cus = 0;
    DeviceBuffers buf;
    // Pass overlap: a second set of everything a pass writes (its `pixels` stays null: the list is read-only and shared), made by the first
    // render whose plan has two passes; the stream the odd passes run on; the events that order the two streams (DEP_*), made once and recorded again and again
    DeviceBuffers buf2;
    hipStream_t pass_stream = nullptr;
    std::vector<hipEvent_t> pass_deps;
    AdaptiveBuffers adaptive;        // pt_render_adaptive's, kept between calls like buf
    std::vector<hipEvent_t> events, events2;  // the timing events of the caller's stream and of pass_stream: one per launch boundary, grown on demand
    GrowBuf film_cache;            // pt_render's device film, kept between calls
    GrowBuf spectral_cache;        // pt_render_spectral's device planes (bins x width x height), kept between calls
    // The resident spectral film (pt_spectral_project_resident): what the last successful spectral render left in spectral_cache.  Cleared when a spectral render
    // starts and set when it has succeeded; pt_render_spectral and pt_render_adaptive_spectral are the only writers of spectral_cache (its reserve, which
    // may replace it, runs inside them behind the clearing).
    bool spectral_valid = false;
    uint32_t spectral_width = 0, spectral_height = 0, spectral_bins = 0;
    // After a node render (pt_render_spectral_multi / pt_render_adaptive_spectral_multi) the resident film is the set of packed shards instead: spectral_shards
    // (on the scene the call was made on) names the scenes that hold them — this one and its replicas, which live as long as it does; empty = spectral_cache.
    // Each of those scenes keeps its own shard, spectral_shard: spectral_bins planes of floats.
    std::vector<pt_scene*> spectral_shards;
    Shard spectral_shard;
    // The resident group films (include/pt_light_groups.h): what the last successful light-group render left in group_films_cache, group-major float4 films.  Cleared
    // when a group render starts and set when it has succeeded; the group renders (a node render's worker on its own scene or replica among them) and the group part of
    // pt_resident_assemble are the only writers of the buffer.  group_table: that render's one byte per
    // instance; group_mix_cache: pt_light_groups_mix_resident's device matrices (PT_LIGHT_GROUPS_MAX x 9 floats) and, behind them, its output film.
    bool groups_valid = false;
    uint32_t groups_width = 0, groups_height = 0, groups_count = 0;
    GrowBuf group_films_cache, group_table, group_mix_cache;
    // After a node group render (include/pt_light_groups_multi.h) the resident group films are the set of packed shards instead: group_shards (on the scene the call
    // was made on) names the scenes that hold them — this one and its replicas; empty = group_films_cache.  Each of those scenes keeps its own shard,
    // group_shard: groups_count films of float4.  A shard of its own, list included: a spectral node render's shard, resident at the same time, may be of
    // another film size.
    std::vector<pt_scene*> group_shards;
    Shard group_shard;
    // The resident group bins (include/pt_light_groups_spectral.h): what the last successful pt_render_light_groups_spectral left in group_bins_cache, group-major, then
    // bin-major planes of width * height floats.  Cleared when a group render of any kind starts (the other two leave none) and set when that render has succeeded;
    // it is the only writer of the buffer.  relamp_cache: pt_light_groups_relamp_resident's device matrix (PT_SPECTRAL_MAX_RESPONSES x 512 floats) and, behind it,
    // its output planes.
    bool group_bins_valid = false;
    uint32_t group_bins_width = 0, group_bins_height = 0, group_bins_groups = 0, group_bins_bins = 0;
    GrowBuf group_bins_cache, relamp_cache;
    // include/pt_light_groups_denoise.h.  groups_paired: the group films and the resident FILM came from one render (pt_render_adaptive_light_groups); ended where the
    // resident film is ended or replaced and where another group render starts.  groups_denoised: pt_denoise_light_groups_resident has left denoised group films in
    // group_den_films (of groups_width x groups_height x groups_count, beside its film and variance in group_den_film / group_den_var: pt_denoise_resident's
    // outputs are not touched); cleared when a group render of either kind or that entry starts.  group_dn_buf: the passes' two ping-pong group buffers.
    bool groups_paired = false, groups_denoised = false;
    GrowBuf group_dn_buf[2], group_den_films, group_den_film, group_den_var;
    ResidentSet resident;          // include/pt_resident.h
    GrowBuf assemble_staging, assemble_px;   // pt_resident_assemble's: the packed shards copied from other devices, and the pixel lists uploaded for the unpack
    GrowBuf project_cache;         // pt_spectral_project_resident's device matrix (PT_SPECTRAL_MAX_RESPONSES x PT_SPECTRAL_MAX_BINS floats) and, behind it, its output planes
    // The resident matte (include/pt_denoise.h, the ID mattes): the keys and the coverage the last successful pt_render_mattes left in matte_keys and matte_coverage,
    // matte_ranks planes of matte_width x matte_height each.  Buffers of their own, outside the resident set's parts: no film render reads or writes them.  Cleared
    // when a matte render starts and set when it has succeeded.  matte_extract_cache: pt_matte_extract_resident's selections (ptk::kMatteSelectionWords words) and,
    // behind them, its output planes.
    bool mattes_valid = false;
    uint32_t matte_width = 0, matte_height = 0, matte_ranks = 0, matte_samples = 0;
    GrowBuf matte_keys, matte_coverage, matte_extract_cache;
    std::vector<pt_scene*> replicas; // pt_render_multi: this scene on the other (virtual) devices, by device index x virtual index (nullptr = not made yet / this one)
};

// The two kinds of packed shard (pt_shard_rules.h): the element in floats, which of a scene's shards holds it, and which full-size buffer a render writes
// and the pack kernel reads.
struct ShardKind {
    uint32_t floats;
    Shard pt_scene::*shard;
    GrowBuf pt_scene::*full;
};
static const ShardKind kSpectralShard = {1u, &pt_scene::spectral_shard, &pt_scene::spectral_cache};
static const ShardKind kGroupShard = {4u, &pt_scene::group_shard, &pt_scene::group_films_cache};
// a shard's packed planes back into full-size planes on the host, by the element of the kind
static void shard_scatter_host(const ShardKind& kind, const void* packed, const std::vector<uint32_t>& px, uint32_t planes, float* full, size_t full_pixels) {
    if (kind.floats == 1) ptd::shard_scatter(static_cast<const float*>(packed), px.data(), (uint32_t)px.size(), planes, full, full_pixels);
    else ptd::shard_scatter(static_cast<const ptd::ShardPixel*>(packed), px.data(), (uint32_t)px.size(), planes, reinterpret_cast<ptd::ShardPixel*>(full), full_pixels);
}

namespace {
std::string g_device_info;

pt_status no_device() { return fail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback"); }
pt_status ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return no_device();
    return PT_OK;
}

// Segment capacity for n items over `grid` segments, rounded up to 64 items so that every segment starts on a
// 256-byte boundary in every field.
uint32_t segment_capacity(uint32_t n, int grid) {
    uint32_t c = (n + (uint32_t)grid - 1) / (uint32_t)grid;
    return (c + 63u) & ~63u;
}

// `b`: the scene's first set or its second (n_pixels 0: no pixel list of its own).  need_hits: the plan is not fused (a fused plan never touches the hit queue,
// 5.9 GB at 128 Mi slots: it is made by the first render that needs it).
// group_planes: the light groups of the render (0: none) — their energy planes lie behind the total and the wavelength samples — and, for a path-pass render,
// the plane of state words behind its eight class planes (pt_path_pass_rules.h).
pt_status ensure_buffers(pt_scene* sc, DeviceBuffers& b, uint32_t capacity, uint32_t light_samples, size_t n_pixels, int grid, uint32_t nl, uint32_t park_block, bool need_hits,
                         uint32_t group_planes) {
    uint32_t total = segment_capacity(capacity, grid) * (uint32_t)grid;
    const uint32_t planes_wanted = group_planes ? lg_planes(group_planes) : nl + 1u;
    if (b.capacity < total || b.light_samples < light_samples || b.grid != grid || b.nl < nl || b.park_block < park_block || b.energy_planes < planes_wanted) {
        hipFree(b.paths_a); hipFree(b.paths_b); hipFree(b.hits); hipFree(b.shadow); hipFree(b.energy); hipFree(b.counts); hipFree(b.block_stats); hipFree(b.park);
        b.paths_a = b.paths_b = b.hits = b.shadow = b.counts = b.park = nullptr; b.energy = nullptr; b.block_stats = nullptr; b.capacity = 0;
        uint32_t ls = light_samples > b.light_samples ? light_samples : b.light_samples;
        uint32_t nlmax = nl > b.nl ? nl : b.nl;
        size_t path_fields = nlmax == 4 ? Layout<4>::path_fields : Layout<1>::path_fields;
        size_t sh_fields = nlmax == 4 ? Layout<4>::shadow_queue_fields(ls ? ls : 1) : Layout<1>::shadow_queue_fields(ls ? ls : 1);
        HIP_TRY(hipMalloc(&b.paths_a, sizeof(uint32_t) * path_fields * total));
        HIP_TRY(hipMalloc(&b.paths_b, sizeof(uint32_t) * path_fields * total));
        HIP_TRY(hipMalloc(&b.shadow, sizeof(uint32_t) * sh_fields * total));
        uint32_t planes = nlmax + 1u;   // (+ the plane of wavelength samples, PT_STORED_WAVELENGTH)
        for (uint32_t want : {b.energy_planes, planes_wanted}) if (want > planes) planes = want;
        HIP_TRY(hipMalloc(&b.energy, sizeof(float) * (size_t)planes * total));
        b.nl = nlmax; b.energy_planes = planes;
        HIP_TRY(hipMalloc(&b.counts, sizeof(uint32_t) * 4 * (size_t)grid));   // (live paths x 2, light-sample items, live light-sample items)
        HIP_TRY(hipMalloc(&b.block_stats, sizeof(unsigned long long) * BS_FIELDS * (size_t)grid));
        // (the parked kernels' scratch: scenes whose sweep table holds walked meshes, and every scene without a sweep table — with or without a mesh: the parked
        // kernels over the top-level tree list their live rays and run at five / four waves per SIMD, and beat the per-lane walk kernels even where no ray ever
        // parks: test_bokeh.toml + a floor, k_extend 1265 -> 693 us, k_shadow 5948 -> 2887 us, profiles/r5_experiments.md section 1)
        const bool no_table = sc->host.blob[PT_HDR_SWEEP_OFF] == 0 || (sc->host.blob[PT_HDR_FLAGS] & PT_FLAG_NO_SWEEP);
        if ((sc->host.blob[PT_HDR_FLAGS] & PT_FLAG_SWEEP_WALKS) || no_table)
            HIP_TRY(hipMalloc(&b.park, sizeof(uint32_t) * kParkFields * (kParkCap / (kBlock / 64)) * (park_block / 64) * (size_t)grid));   // (128 entries per wave)
        b.park_block = park_block;
        if (!b.unit_counters) HIP_TRY(hipMalloc(&b.unit_counters, sizeof(uint32_t) * kUnitCounters));
        b.capacity = total; b.light_samples = ls; b.grid = grid;
    }
    if (need_hits && !b.hits) HIP_TRY(hipMalloc(&b.hits, sizeof(uint32_t) * (size_t)HS_FIELDS * b.capacity));
    if (b.pixel_capacity < n_pixels) {
        hipFree(b.pixels); b.pixels = nullptr;
        HIP_TRY(hipMalloc(&b.pixels, sizeof(uint32_t) * n_pixels));
        b.pixel_capacity = n_pixels;
    }
    return PT_OK;
}

pt_status ensure_adaptive_buffers(pt_scene* sc, size_t n_pixels) {
    AdaptiveBuffers& a = sc->adaptive;
    if (a.pixels >= n_pixels) return PT_OK;
    a.release();
    const size_t blocks = (n_pixels + kBlock - 1) / kBlock;
    HIP_TRY(hipMalloc(&a.counts, sizeof(uint32_t) * n_pixels));
    HIP_TRY(hipMalloc(&a.lists[0], sizeof(uint32_t) * n_pixels));
    HIP_TRY(hipMalloc(&a.lists[1], sizeof(uint32_t) * n_pixels));
    HIP_TRY(hipMalloc(&a.block_counts, sizeof(uint32_t) * (blocks + 1)));
    HIP_TRY(hipMalloc(&a.stats, sizeof(double) * 2 * n_pixels));
    HIP_TRY(hipMalloc(&a.unconverged, n_pixels));
    a.pixels = n_pixels;
    return PT_OK;
}

template <typename K, typename... Args>
void launch(K kernel, uint32_t lds_bytes, int grid, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds_bytes, stream, args...);
}

uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return (uint32_t)strtoul(v, nullptr, 10);
}
// The worker threads of a node call (pt_render_adaptive_multi) meet here between the steps of a round.  The last one to arrive runs the step that needs
// every device (the exchange, the stop decision) while the others wait.  A worker that fails calls stop(): every worker waiting or arriving later is released
// with false, so that no thread enters a collective after another has failed, and the first error is kept for the caller.  (C++17: no std::barrier.)
struct Lockstep {
    std::mutex mu;
    std::condition_variable cv;
    int parties = 0, waiting = 0;
    uint64_t generation = 0;
    bool failed = false;
    pt_status status = PT_OK;
    std::string error;
    void stop(pt_status st, const std::string& msg) {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed) { failed = true; status = st; error = msg; }
        cv.notify_all();
    }
    // `last`: run by the last worker to arrive, with every other one waiting (the lock held); its failure stops them all (message in g_error)
    bool arrive(const std::function<pt_status()>& last) {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return false;
        const uint64_t gen = generation;
        if (++waiting == parties) {
            waiting = 0;
            const pt_status st = last();
            if (st != PT_OK && !failed) { failed = true; status = st; error = g_error; }
            ++generation;
            cv.notify_all();
            return !failed;
        }
        cv.wait(lk, [&] { return failed || generation != gen; });
        return !failed;
    }
};

// What the workers of pt_render_adaptive_multi share.  images[v]: virtual device v's unconverged image; merged[v]: the film-wide image its keep reads (the
// image of the first virtual device on its physical device, where `exchange` merges them).  next[v]: the length of v's next list; total: their sum.
struct NodeRounds {
    Lockstep lock;
    std::function<pt_status()> exchange;
    std::vector<uint8_t*> images;
    std::vector<const uint8_t*> merged;
    std::vector<uint32_t> next;
    uint64_t total = 0;
    double exchange_seconds = 0.0;
};

// The rounds of pt_render_adaptive (include/pt_adaptive.h) on render_impl's pass loop `run(list, n, first_sample, sample_count, stats)`:
// round 0 renders samples [0, spp) of the n0 pixels in lists[0], every later round the next `step` samples of the pixels the round before kept.  The one
// read-back of a round is the length of the next list (4 bytes): it plans that round's passes.  With `node` (pt_render_adaptive_multi, worker v) the
// rounds run in lockstep with the other devices: after the marks the images are merged into the film-wide one that every device's keep reads, and the
// rounds end when no device's next list holds a pixel.  A device whose list is empty goes on taking part with an all-zero image.
template <typename RunPasses>
pt_status adaptive_rounds(pt_scene* sc, const pt_render_desc& rd, const pt_adaptive_desc& ad, hipStream_t stream, float* d_film, uint32_t n0, RunPasses&& run,
                          uint32_t* rounds, NodeRounds* node, int v) {
    AdaptiveBuffers& a = sc->adaptive;
    const uint32_t film_pixels = rd.width * rd.height;
    const int small_grid = sc->num_cus * 4;
    uint32_t n = n0, c = 0, len = rd.spp, cur = 0;
    const auto stopped = [] { return fail(PT_ERR_DEVICE, "stopped: another device of the node failed"); };
    for (*rounds = 0;;) {
        pt_status st = run(a.lists[cur], n, c, len, a.stats);
        if (st != PT_OK) return st;
        c += len;
        ++*rounds;
        HIP_TRY(hipMemsetAsync(a.unconverged, 0, film_pixels, stream));
        hipLaunchKernelGGL(k_adaptive_mark, dim3(small_grid), dim3(kBlock), 0, stream, a.lists[cur], n, c, a.stats, ad.rel_error, ad.abs_error, a.counts, a.unconverged);
        if (c >= ad.max_samples) break;
        const uint8_t* unconverged = a.unconverged;
        if (node) {   // the exchange: every device has marked its own pixels
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(stream));
            if (!node->lock.arrive(node->exchange)) return stopped();
            unconverged = node->merged[v];
        }
        uint32_t next = 0;
        if (n > 0) {
            const uint32_t nb = (n + kBlock - 1) / kBlock;
            hipLaunchKernelGGL(k_adaptive_keep, dim3(nb), dim3(kBlock), 0, stream, a.lists[cur], n, c, ad.max_samples, unconverged, rd.width, rd.height, a.block_counts);
            hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(kBlock), 0, stream, a.block_counts, nb);
            hipLaunchKernelGGL(k_adaptive_scatter, dim3(nb), dim3(kBlock), 0, stream, a.lists[cur], n, c, ad.max_samples, unconverged, rd.width, rd.height,
                               a.block_counts, a.lists[cur ^ 1u]);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&next, a.block_counts + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        uint64_t total = next;
        if (node) {   // the decision: the sum of every device's next length
            node->next[v] = next;
            if (!node->lock.arrive([node] { node->total = 0; for (uint32_t k : node->next) node->total += k; return PT_OK; })) return stopped();
            total = node->total;
        }
        if (total == 0) break;
        n = next;
        cur ^= 1u;
        len = ad.step < ad.max_samples - c ? ad.step : ad.max_samples - c;
    }
    hipLaunchKernelGGL(k_adaptive_finish, dim3(small_grid), dim3(kBlock), 0, stream, film_pixels, a.counts, d_film);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// What is optional about a render (render_impl): a default-constructed job is pt_render's.
struct RenderJob {
    // pt_render_adaptive (its arguments checked): adaptive_rounds runs the pass loop once per round, over the film or (with `node`: worker node_index of
    // pt_render_adaptive_multi) over the desc's shard
    const pt_adaptive_desc* adaptive = nullptr;
    NodeRounds* node = nullptr;
    int node_index = 0;
    // pt_render_spectral (its arguments checked): spectral_bins planes of width * height floats; every pass also adds its samples to the wavelength-binned film
    // (include/pt_spectral.h).  With `adaptive` too (pt_render_adaptive_spectral and its node form) the bins hold running sums, a continued pixel starting from its
    // stored value, until k_adaptive_finish_spectral divides each pixel's by its own count.
    float* d_spectral = nullptr;
    uint32_t spectral_bins = 0;
    // the spectral node entries: the desc's shard as pth::shard_pixels lists it, computed by the caller, who packs the bins by it afterwards — the device copy of it
    // is then left in the scene's buf.pixels whichever kind of render this is
    const std::vector<uint32_t>* shard_list = nullptr;
    // pt_render_light_groups (its arguments checked; include/pt_light_groups.h): the group table, its bytes in device memory, and group_count films of width * height
    // float4 — the render takes the general vertex and light-sample forms that route energy to the groups' planes, and every pass adds each plane to its film
    const LightGroupTable* groups = nullptr;
    float* d_group_films = nullptr;
    // pt_render_path_passes (its arguments checked; include/pt_light_groups.h): a group render of PP_CLASSES films whose vertex and light-sample forms route the
    // energy by the path's own history (PassRouter, pt_path_pass_rules.h) and keep a plane of state words behind the class planes; d_group_films as above, no table
    bool classes = false;
    // pt_render_path_exprs (its arguments checked; include/pt_light_groups.h "Path expressions"): a group render of exprs->outputs films routed by the program's
    // automaton (ExprRouter, pt_path_expr_rules.h), with a plane of state words behind the expression planes as a pass render has; d_expr_table: the program's 64
    // entries in device memory, d_expr_groups: one light group id per instance there, or null; d_group_films as above
    const pt_path_expr_program* exprs = nullptr;
    const PxEntry* d_expr_table = nullptr;
    const uint8_t* d_expr_groups = nullptr;
    // pt_render_light_groups_spectral (include/pt_light_groups_spectral.h): with groups and d_spectral, group_count * spectral_bins planes of width * height floats —
    // every pass also adds each group's plane to that group's bins
    float* d_group_bins = nullptr;
};

// The plan of a render (pth::plan_render: host logic alone, pinned by tests/golden/render_plans.tsv) from what the scene and the job hold, and — a measurement
// build only — the arms that read the environment, applied to the finished plan.  *live_lists: LaunchCfg's field of that name.
pt_status plan_for(const pt_scene* sc, const pt_render_desc& rd, const RenderJob& job, size_t n_pixels, pth::RenderPlan* plan, bool* live_lists) {
    pth::RenderAsk ask;
    ask.num_cus = sc->num_cus; ask.rd = rd; ask.n_pixels = n_pixels; ask.adaptive = job.adaptive;
    ask.routed = job.groups != nullptr || job.classes || job.exprs != nullptr;
#ifdef PT_EXPERIMENTS
    ask.pool_lds_bytes = pool_lds_bytes();
#endif
    std::string err;
    if (!pth::plan_render(sc->host.blob, sc->tuning, pth::ScenePlan{sc->lacks, sc->lds_mode}, ask, plan, &err)) return fail(PT_ERR_INVALID_ARGUMENT, err);
    *live_lists = false;
#ifdef PT_EXPERIMENTS
    *live_lists = env_u32("PT_AMD_LIVE_LISTS", 0) != 0;   // (k_shadow_live: a measurement build's kernel, profiles/r4_experiments.md)
    // a measurement build runs the shipped kernel pair unless one of its own forms is asked for: those read every item of a segment
    if (*live_lists || getenv("PT_AMD_EXP_SHADOW")) plan->live_list = 0u;
#endif
    return PT_OK;
}
// The one place a launch configuration is made from a plan (unit_counter and path_marks are the pass loop's, per launch; so is the stream of a pass on the second lane)
LaunchCfg launch_cfg(const pt_scene* sc, const pth::RenderPlan& plan, bool live_lists, hipStream_t stream) {
    LaunchCfg cfg{plan.grid, plan.lds_bytes, stream, sc->lds_mode};
    cfg.dyn_grid = plan.dyn_grid;
    cfg.lacks = sc->lacks;
    cfg.walk_policy = plan.walk_policy;
    cfg.park_block = plan.launch_park_block; cfg.park_block_extend = plan.launch_park_block_extend; cfg.park_blob_bytes = plan.park_blob_bytes;
    cfg.live_lists = live_lists;
    cfg.certs = plan.certs;
    cfg.mesh_lights = plan.mesh_lights;
    cfg.fuse = plan.fuse;
    return cfg;
}

// The stage clock of a render: HIP events around every launch, recorded on the launch stream and read back after the final sync, so the
// per-stage device time is measured inside the timed region without stalling it.
// (round 5: ONE event between two launches — the end of one is the start of the next on the stream — not two: the markers cost a short frame 5 % of its time,
// G2 9.7 -> 9.2 ms per step without any; a launch's time now includes the gap in front of it, a few microseconds)
// (pass overlap: each lane of the pass loop keeps its own chain; a wait for the other stream gets an event of its own behind it, so that the idle time is charged to no stage)
struct StageClock {
    struct Chain {
        hipStream_t stream; std::vector<hipEvent_t>* events;   // the lane's stream and the scene's events for it, grown on demand
        size_t marks;              // timing events recorded
        std::vector<int> stage;    // stage[k]: what the interval from event k to event k + 1 is charged to (-1: no stage)
    };
    Chain chain[2];
    bool ok;   // the tuning asks for timing and no event call has failed
    double ms[ST_COUNT] = {0, 0, 0, 0, 0};
    uint64_t launches[ST_COUNT] = {0, 0, 0, 0, 0};
    // an event behind what the lane's stream holds so far: the interval since the lane's previous one is charged to `stage`
    void mark(uint32_t lane, int stage) {
        Chain& l = chain[lane];
        if (!ok) return;
        while (l.events->size() <= l.marks) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { ok = false; return; } l.events->push_back(e); }
        if (hipEventRecord((*l.events)[l.marks], l.stream) != hipSuccess) { ok = false; return; }
        if (l.marks > 0) l.stage.push_back(stage);
        ++l.marks;
    }
    template <typename Fn> void timed(uint32_t lane, int stage, Fn&& fn) {
        fn();
        mark(lane, stage);
        launches[stage]++;
    }
    // behind the final synchronise: every charged interval into ms; overlapped: some pass loop of the render ran passes on both lanes
    void read(bool overlapped) {
        for (const Chain& l : chain) for (size_t k = 0; k < l.stage.size(); ++k) {
            float t = 0.0f;
            if (l.stage[k] >= 0 && hipEventElapsedTime(&t, (*l.events)[k], (*l.events)[k + 1]) == hipSuccess) ms[l.stage[k]] += t;
        }
        if (!overlapped || chain[0].marks == 0) return;
        // (pt_profile::kernel_seconds: overlapped intervals add up to more than the device was busy, so each stage gets its share of the busy window, the first
        // timing event to the last over both streams)
        double window = 0.0, total = 0.0;
        for (const Chain& l : chain) {
            float t = 0.0f;
            if (l.marks > 0 && hipEventElapsedTime(&t, (*chain[0].events)[0], (*l.events)[l.marks - 1]) == hipSuccess && t > window) window = t;
        }
        for (double t : ms) total += t;
        if (window > 0.0 && total > window) for (double& t : ms) t *= window / total;
    }
};

// A render's profile: the workgroups' counters read back and summed, beside what the pass loop counted and the clock timed on the host.
pt_status read_profile(pt_scene* sc, const pth::RenderPlan& plan, bool second_set, uint64_t camera_rays, uint64_t accumulated_pixels, const StageClock& clock,
                       uint32_t rounds, double seconds, pt_profile* profile) {
    memset(profile, 0, sizeof(*profile));
    std::vector<unsigned long long> bs((size_t)plan.grid * BS_FIELDS);
    unsigned long long c[BS_FIELDS] = {0, 0, 0, 0, 0, 0};
    for (const unsigned long long* d_bs : {(const unsigned long long*)sc->buf.block_stats, (const unsigned long long*)(second_set ? sc->buf2.block_stats : nullptr)}) {   // (each set's workgroups count into their own)
        if (!d_bs) continue;
        HIP_TRY(hipMemcpy(bs.data(), d_bs, sizeof(unsigned long long) * bs.size(), hipMemcpyDeviceToHost));
        for (int g = 0; g < plan.grid; ++g) for (int k = 0; k < BS_FIELDS; ++k) c[k] += bs[(size_t)g * BS_FIELDS + k];
    }
    profile->camera_rays = camera_rays;
    profile->bounce_rays = c[BS_VERTICES] + camera_rays;  // vertices.len() counts the camera vertex (utils.rs:375)
    profile->shadow_rays = c[BS_SHADOW_RAYS];
    profile->env_hits = c[BS_ENV_HITS];
    profile->seconds = seconds;
    for (int i = 0; i < ST_COUNT; ++i) { profile->kernel_seconds[i] = clock.ms[i] * 1e-3; profile->kernel_launches[i] = clock.launches[i]; }
    profile->stage_items[ST_GENERATE] = camera_rays; profile->stage_items[ST_EXTEND] = c[BS_SEGMENTS]; profile->stage_items[ST_SHADE] = c[BS_SEGMENTS];
    profile->stage_items[ST_SHADOW] = c[BS_ITEMS]; profile->stage_items[ST_ACCUMULATE] = accumulated_pixels;
    profile->stage_items[6] = (uint64_t)plan.launch_park_block;   // threads per workgroup of the parked kernels when they ran in their big-workgroup form (pt_tuning::park_block), else 0
    profile->stage_items[7] = plan.camera_record;   // 1: k_generate wrote the camera vertex' lean record (7 of 16 words) and the first bounce's vertex kernel rebuilt the rest
    profile->stage_items[5] = c[BS_MEDIUM_DROPS];   // the medium-aware walk tracks four nested mediums: what a fifth level lost (0 = the walk is the reference's)
    profile->kernel_launches[5] = rounds;           // pt_render_adaptive: its rounds (0 for pt_render)
    return PT_OK;
}

// The events that order the two streams of overlapped passes (pt_scene::pass_deps): the fork, and per pass parity the accumulate stage done and the skew bounce done
enum { DEP_FORK = 0, DEP_ACCUMULATED = 1, DEP_SKEW = 3, DEP_COUNT = 5 };

// Pass overlap: a render whose plan wants it (pth::RenderPlan::overlap: its pass loop plans two passes or more somewhere) gets the second set of pass buffers, sized
// as ensure_buffers sized the first, the second stream and the events between the two.  Where the device cannot give them, what was taken is given back and the
// passes run one after the other as before: that is no error of the call.  Returns whether passes overlap.
bool acquire_second_lane(pt_scene* sc, const pth::RenderPlan& plan, uint32_t light_samples, uint32_t nl, bool need_hits, uint32_t group_planes) {
    if (!plan.overlap) return false;
    bool ok = ensure_buffers(sc, sc->buf2, plan.capacity, light_samples, 0, plan.grid, nl, plan.park_block, need_hits, group_planes) == PT_OK;
    if (ok && !sc->pass_stream) ok = hipStreamCreateWithFlags(&sc->pass_stream, hipStreamNonBlocking) == hipSuccess;
    while (ok && sc->pass_deps.size() < DEP_COUNT) {
        hipEvent_t e;
        ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (ok) sc->pass_deps.push_back(e);
    }
    if (!ok) { sc->buf2.release(); (void)hipGetLastError(); }   // (the sticky error cleared)
    return ok;
}

// What the kernels of a render read of the desc and the plan; the pass loop fills in what changes per pass (the chunk, the sample range, the set's energy_stride)
RenderParams render_params(const pt_scene* sc, const pt_render_desc& rd, const pt_adaptive_desc* adaptive, const pth::RenderPlan& plan) {
    RenderParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.seed = rd.seed; rp.width = rd.width; rp.height = rd.height;
    rp.min_bounces = rd.min_bounces; rp.max_bounces = rd.max_bounces; rp.light_samples = rd.light_samples; rp.only_direct = rd.only_direct;
    rp.wavelength_lo = rd.wavelength_lo; rp.wavelength_span = rd.wavelength_hi - rd.wavelength_lo;
    // (an adaptive render's film holds running sums until k_adaptive_finish divides each pixel by its own count; its rounds end on phase boundaries)
    rp.spp = adaptive ? adaptive->max_samples : rd.spp; rp.range_end = rd.first_sample + rd.sample_count;
    rp.normalize = (!adaptive && rd.first_sample == 0 && rd.sample_count == rd.spp) ? 1u : 0u;
    rp.phase = rd.phase_samples;
    rp.camera = pth::camera_params(sc->host.cameras[rd.camera_index], (float)rd.width / (float)rd.height);
    rp.live_list = plan.live_list; rp.camera_record = plan.camera_record;
    return rp;
}

// A render in four steps: the plan (pth::plan_render), the buffers and the upload of the pixel list, the pass loop — pt_render runs it once over its shard's
// pixels, an adaptive job once per round (adaptive_rounds) —, timed by the stage clock, and the profile (read_profile).  `job`: what is optional about the render.
pt_status render_impl(pt_scene* sc, const pt_render_desc* rdp, float* d_film, hipStream_t stream, pt_profile* profile, const RenderJob& job) {
    if (!sc || !rdp || !d_film) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    pt_render_desc rd;
    std::string err;
    if (!pth::normalize_render_desc(*rdp, (uint32_t)sc->host.cameras.size(), &rd, &err)) return fail(PT_ERR_INVALID_ARGUMENT, err);
    HIP_TRY(hipSetDevice(sc->device));

    const pt_adaptive_desc* adaptive = job.adaptive;
    std::vector<uint32_t> own_list;
    if (!job.shard_list) own_list = pth::shard_pixels(rd.width, rd.height, rd.tile_width, rd.tile_height, rd.shard_index, rd.shard_count);
    const std::vector<uint32_t>& pixels = job.shard_list ? *job.shard_list : own_list;
    pth::RenderPlan plan;
    bool live_lists = false;
    pt_status st = plan_for(sc, rd, job, pixels.size(), &plan, &live_lists);
    if (st != PT_OK) return st;
    const int grid = plan.grid;
    const bool hero = plan.hero, parked_form = plan.trav_form == PT_FORM_PARKED || plan.trav_form == PT_FORM_PARKED_WALK;
    LaunchCfg cfg = launch_cfg(sc, plan, live_lists, stream);

#ifdef PT_EXPERIMENTS
    const bool need_hits = true;   // (the measurement forms of k_shadow keep scratch in the idle hit queue, fused plan or not)
#else
    const bool need_hits = !plan.fuse;
#endif
    const uint32_t group_count = job.classes ? PP_CLASSES : job.exprs ? job.exprs->outputs : job.groups ? job.groups->group_count : 0u;
    const uint32_t group_planes = group_count + (job.classes || job.exprs ? 1u : 0u);   // (+ the plane of state words)
    const uint32_t nl = (hero || rd.medium_aware) ? 4u : 1u;
    st = ensure_buffers(sc, sc->buf, plan.capacity, rd.light_samples, pixels.size() ? pixels.size() : 1, grid, nl, plan.park_block, need_hits, group_planes);
    if (st != PT_OK) return st;
    DeviceBuffers& b = sc->buf;
    const bool overlap = acquire_second_lane(sc, plan, rd.light_samples, nl, need_hits, group_planes);
    if (overlap && parked_form && !sc->buf2.park) return fail(PT_ERR_DEVICE, "internal: a parked traversal form without the second set's scratch");
    if (parked_form && !b.park) return fail(PT_ERR_DEVICE, "internal: a parked traversal form without the parked kernels' scratch");
    if (adaptive) {   // (round 0's list: every pixel of the film — or of the shard — in shard_pixels' order; counts and stats are zero outside it)
        const size_t film_pixels = (size_t)rd.width * rd.height;
        st = ensure_adaptive_buffers(sc, film_pixels);
        if (st != PT_OK) return st;
        if (!pixels.empty()) HIP_TRY(hipMemcpyAsync(sc->adaptive.lists[0], pixels.data(), sizeof(uint32_t) * pixels.size(), hipMemcpyHostToDevice, stream));
        // (the rounds compact into lists[0] again: the list the caller packs by is kept where pt_render keeps its own)
        if (job.shard_list && !pixels.empty()) HIP_TRY(hipMemcpyAsync(b.pixels, pixels.data(), sizeof(uint32_t) * pixels.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(sc->adaptive.stats, 0, sizeof(double) * 2 * film_pixels, stream));
        if (pixels.size() < film_pixels) HIP_TRY(hipMemsetAsync(sc->adaptive.counts, 0, sizeof(uint32_t) * film_pixels, stream));
    } else if (!pixels.empty()) HIP_TRY(hipMemcpyAsync(b.pixels, pixels.data(), sizeof(uint32_t) * pixels.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_film, 0, sizeof(float) * 4 * (size_t)rd.width * rd.height, stream));
    if (job.d_spectral) HIP_TRY(hipMemsetAsync(job.d_spectral, 0, sizeof(float) * (size_t)job.spectral_bins * rd.width * rd.height, stream));
    if (group_count) HIP_TRY(hipMemsetAsync(job.d_group_films, 0, sizeof(float) * 4 * (size_t)group_count * rd.width * rd.height, stream));
    if (job.d_group_bins) HIP_TRY(hipMemsetAsync(job.d_group_bins, 0, sizeof(float) * (size_t)group_count * job.spectral_bins * rd.width * rd.height, stream));
    HIP_TRY(hipMemsetAsync(b.block_stats, 0, sizeof(unsigned long long) * BS_FIELDS * (size_t)grid, stream));
    if (overlap) HIP_TRY(hipMemsetAsync(sc->buf2.block_stats, 0, sizeof(unsigned long long) * BS_FIELDS * (size_t)grid, stream));   // (in front of the fork event)

    RenderParams rp = render_params(sc, rd, adaptive, plan);
    const pt_tuning& tn = sc->tuning;
    const SceneArgs sargs{sc->d_blob, sc->blob_words, sc->d_tex, marginal_lds_bytes(sc->host.blob.data(), cfg.lds_bytes)};
    const uint32_t bounce_limit = rd.only_direct ? 1u : rd.max_bounces;
    // A lane of the pass loop: a set of pass buffers and the stream its passes run on (the clock's chain of the same index times it).  Lane 0 is the first set on
    // the caller's stream; lane 1 (overlap only) the second set on the scene's own stream.
    struct Lane {
        DeviceBuffers* set; hipStream_t stream;
        Queue qa, qb, qh, qs;
        uint32_t* live[2];         // per-segment live-path counts, ping-pong with the path queues
        uint32_t* nshadow;         // per-segment light-sample item counts; behind them (nshadow + grid) the counts of the live ones (Layout::shadow_live_field)
        PassRouter pass_router;    // a path-pass render: the router over the set's state plane
        ExprRouter expr_router;    // a path-expression render: likewise, behind its own number of planes
    };
    auto make_lane = [&](DeviceBuffers& s, hipStream_t on) {
        return Lane{&s, on, Queue{s.paths_a, s.capacity, plan.path_fields}, Queue{s.paths_b, s.capacity, plan.path_fields}, Queue{s.hits, s.capacity, HS_FIELDS},
                    Queue{s.shadow, s.capacity, plan.item_fields}, {s.counts, s.counts + grid}, s.counts + 2 * grid,
                    PassRouter{job.classes ? pp_state_words(s.energy, s.capacity) : nullptr},
                    ExprRouter{{job.d_expr_table, job.d_expr_groups, job.exprs ? px_state_words(s.energy, s.capacity, job.exprs->outputs) : nullptr, job.exprs ? job.exprs->start : 0u}}};
    };
    const GroupRouter group_router{job.groups ? *job.groups : LightGroupTable{nullptr, 0u, 0u}};
    Lane lanes[2] = {make_lane(b, stream), make_lane(overlap ? sc->buf2 : b, overlap ? sc->pass_stream : stream)};

    HIP_TRY(hipStreamSynchronize(stream));
    const auto t0 = std::chrono::steady_clock::now();
    StageClock clock{{{lanes[0].stream, &sc->events, 0, {}}, {lanes[1].stream, &sc->events2, 0, {}}}, !(tn.flags & PT_TUNE_NO_STAGE_TIMING)};
    clock.mark(0, -1);

    uint64_t camera_rays = 0, accumulated_pixels = 0;
    hipError_t spectral_error = hipSuccess, groups_error = hipSuccess, group_bins_error = hipSuccess;
    bool overlapped = false;   // some pass loop of this render ran passes on both lanes
    const std::vector<hipEvent_t>& dep = sc->pass_deps;
    const uint32_t skew_code = (tn.flags >> PT_TUNE_PASS_SKEW_SHIFT) & PT_TUNE_PASS_SKEW_MASK;
    const int32_t skew_bounce = skew_code == 0u ? pth::kPassSkewBounce : (int32_t)skew_code - 2;   // (1: -1, the passes start together)
    // The pass loop: samples [first_sample, first_sample + sample_count) of the n pixels of the device list d_list; stats (adaptive rounds): S1 / S2 too
    auto run_passes = [&](const uint32_t* d_list, uint32_t n_list, uint32_t first_sample, uint32_t sample_count, double* d_stats) -> pt_status {
        // (a later adaptive round: the stream's work since the previous accumulate — the round's decision and compaction — is charged to no stage)
        if (camera_rays != 0) clock.mark(0, -1);
        rp.range_end = first_sample + sample_count;
        // the planner's capacity is in items; segments round up, so plan with what surely fits
        std::vector<pth::Pass> passes = pth::plan_passes(n_list, first_sample, sample_count, plan.capacity, rd.phase_samples);
        // which pass runs on which lane, behind which events (pt_plan.h): without overlap, or with one pass, everything on lane 0 and no event
        const pth::PassSchedule sch = pth::schedule_passes((uint32_t)passes.size(), bounce_limit, skew_bounce, overlap);
        const bool two_lanes = sch.steps.size() >= 2 && sch.steps[1].lane == 1u;
        if (two_lanes) { HIP_TRY(hipEventRecord(dep[DEP_FORK], stream)); overlapped = true; }   // (behind whatever the caller's stream holds: an adaptive round's compaction)
        for (size_t p = 0; p < passes.size(); ++p) {
            const pth::Pass& pass = passes[p];
            const pth::PassStep& step = sch.steps[p];
            const uint32_t ln = step.lane;
            const Lane& l = lanes[ln];
            DeviceBuffers& b = *l.set;
            const hipStream_t stream = l.stream;
            const Queue &qa = l.qa, &qb = l.qb, &qh = l.qh, &qs = l.qs;
            uint32_t* const* live = l.live;
            uint32_t* const nshadow = l.nshadow;
            cfg.stream = stream;
            rp.energy_stride = b.capacity;
            accumulated_pixels += pass.pixel_count;
            rp.chunk_pixels = pass.pixel_count; rp.first_sample = pass.first_sample; rp.pass_samples = pass.sample_count;
            uint32_t n = pass.pixel_count * pass.sample_count;
            if (n > b.capacity) return fail(PT_ERR_DEVICE, "internal: a pass of " + std::to_string(n) + " slots exceeds the queue capacity " + std::to_string(b.capacity));
            uint32_t seg_cap = segment_capacity(n, grid);
            camera_rays += n;
            const uint32_t* d_px = d_list + pass.pixel_begin;
            if (step.wait_fork) HIP_TRY(hipStreamWaitEvent(stream, dep[DEP_FORK], 0));
            if (step.start_after >= 0) HIP_TRY(hipStreamWaitEvent(stream, dep[DEP_SKEW + (step.start_after & 1)], 0));
            if (step.wait_fork || step.start_after >= 0) clock.mark(ln, -1);
            if (group_count) {   // (the groups' planes, on the pass's own stream: behind the accumulate stage of the pass that used this set before, in front of this pass's vertices)
                HIP_TRY(hipMemsetAsync(b.energy + (size_t)lg_plane(0) * b.capacity, 0, sizeof(float) * (size_t)group_count * b.capacity, stream));
                clock.mark(ln, -1);
            }
            if (plan.park_dynamic) {
                HIP_TRY(hipMemsetAsync(b.unit_counters, 0, sizeof(uint32_t) * kUnitCounters, stream));
                // (round-5 advisor) an event of its own behind the stream's non-kernel work, charged to no stage: k_generate's time begins here, not at the end of the previous pass
                clock.mark(ln, -1);
            }
            clock.timed(ln, ST_GENERATE, [&] {
                if (hero) hipLaunchKernelGGL(k_generate<4>, dim3(grid), dim3(kBlock), 0, stream, rp, d_px, qa, b.energy, n, seg_cap, live[0]);
                else hipLaunchKernelGGL(k_generate<1>, dim3(grid), dim3(kBlock), 0, stream, rp, d_px, qa, b.energy, n, seg_cap, live[0]);
            });
            for (uint32_t bounce = 0; bounce < bounce_limit; ++bounce) {
                Queue qin = (bounce & 1) ? qb : qa, qout = (bounce & 1) ? qa : qb;
                uint32_t *cin = live[bounce & 1], *cout = live[(bounce + 1) & 1];
                // kernel variant = staging mode (PT_LDS_*) x traversal form x wavelengths per path (pt_launch.h)
                if (plan.park_dynamic) cfg.unit_counter = b.unit_counters + 2 * bounce;
                // (a marked path segment — it left the scene's one certified convex body outward — skips that instance: records the vertex kernel wrote, so from bounce 1 on; never
                // in the medium-aware walk, whose vertex code makes no marks)
                cfg.path_marks = (bounce > 0 && !rd.medium_aware && (sc->host.blob[PT_HDR_FLAGS] & PT_FLAG_CONVEX)) ? sc->host.blob[PT_HDR_CONVEX_INST] : 0u;
                if (!cfg.fuse) clock.timed(ln, ST_EXTEND, [&] { launch_extend(cfg, plan.trav_form, sargs, qin, qh, seg_cap, cin, b.park); });
                if (plan.park_dynamic) cfg.unit_counter = b.unit_counters + 2 * bounce + 1;
                const auto routed = [&](const auto& router) {   // (a routed render's two forms: pt_kern_routed.hip)
                    clock.timed(ln, ST_SHADE, [&] { launch_shade_routed(cfg, sargs, rp, bounce, d_px, qin, qh, qout, qs, b.energy, seg_cap, cin, cout, nshadow, b.block_stats, router); });
                    if (rd.light_samples > 0) clock.timed(ln, ST_SHADOW, [&] { launch_shadow_routed(cfg, sargs, rd.light_samples, qs, b.energy, b.capacity, seg_cap, nshadow, router); });
                };
                if (job.classes) routed(l.pass_router);
                else if (job.exprs) routed(l.expr_router);
                else if (job.groups) routed(group_router);
                else {
                    clock.timed(ln, ST_SHADE, [&] { launch_shade(cfg, hero ? 4 : 1, plan.shade_form, sargs, rp, bounce, d_px, qin, qh, qout, qs, b.energy, seg_cap, cin, cout, nshadow, b.block_stats); });
                    if (rd.light_samples > 0)   // (shade_form FULL = the scene can produce environment rays)
                        clock.timed(ln, ST_SHADOW, [&] { launch_shadow(cfg, plan.trav_form, hero ? 4 : 1, plan.shade_form == PT_SHADE_FULL || plan.shade_form == PT_SHADE_MEDIUM, sargs, rd.light_samples, qs, b.energy, b.capacity, rp.live_list ? (seg_cap | kShadowListed) : seg_cap, nshadow, b.park, qh); });
                }
                // (the next pass starts behind this bounce: started together the two would run in lock step, tail on tail)
                if ((int32_t)bounce == step.signal_bounce) HIP_TRY(hipEventRecord(dep[DEP_SKEW + (p & 1)], stream));
            }
            // (the film sums keep the pass order: phases of 10, pixels continued across passes)
            if (step.accumulate_after >= 0) { HIP_TRY(hipStreamWaitEvent(stream, dep[DEP_ACCUMULATED + (step.accumulate_after & 1)], 0)); clock.mark(ln, -1); }
            clock.timed(ln, ST_ACCUMULATE, [&] {
                if (d_stats && hero) hipLaunchKernelGGL(k_accumulate_stats<4>, dim3(grid), dim3(kBlock), 0, stream, rp, d_px, b.energy, d_film, d_stats);
                else if (d_stats) hipLaunchKernelGGL(k_accumulate_stats<1>, dim3(grid), dim3(kBlock), 0, stream, rp, d_px, b.energy, d_film, d_stats);
                else if (hero) hipLaunchKernelGGL(k_accumulate<4>, dim3(grid), dim3(kBlock), 0, stream, rp, d_px, b.energy, d_film);
                else hipLaunchKernelGGL(k_accumulate<1>, dim3(grid), dim3(kBlock), 0, stream, rp, d_px, b.energy, d_film);
                // (the energy planes stay valid until the next pass's k_generate overwrites them)
                if (job.d_spectral && spectral_error == hipSuccess)
                    spectral_error = ptk::launch_accumulate_spectral(hero ? 4 : 1, grid, stream, rp, d_px, b.energy, job.d_spectral, job.spectral_bins, rd.width * rd.height);
                if (group_count && groups_error == hipSuccess)
                    groups_error = ptk::launch_accumulate_groups(stream, rp, d_px, b.energy, job.d_group_films, group_count, (size_t)rd.width * rd.height);
                if (job.d_group_bins && group_bins_error == hipSuccess)
                    group_bins_error = ptk::launch_accumulate_group_bins(stream, rp, d_px, b.energy, job.d_group_bins, group_count, job.spectral_bins, rd.width * rd.height);
            });
            if (group_bins_error != hipSuccess) return fail(PT_ERR_DEVICE, std::string("k_accumulate_group_bins: ") + hipGetErrorString(group_bins_error));
            if (groups_error != hipSuccess) return fail(PT_ERR_DEVICE, std::string("k_accumulate_groups: ") + hipGetErrorString(groups_error));
            if (spectral_error != hipSuccess) return fail(PT_ERR_DEVICE, std::string("k_accumulate_spectral: ") + hipGetErrorString(spectral_error));
            if (two_lanes) HIP_TRY(hipEventRecord(dep[DEP_ACCUMULATED + (p & 1)], stream));
        }
        // the join: what the caller's stream holds next — an adaptive round's decision, the final synchronise, the caller's own kernels — sees every pass
        if (sch.join_pass >= 0) HIP_TRY(hipStreamWaitEvent(stream, dep[DEP_ACCUMULATED + (sch.join_pass & 1)], 0));
        return PT_OK;
    };
    uint32_t rounds = 0;
    st = adaptive ? adaptive_rounds(sc, rd, *adaptive, stream, d_film, (uint32_t)pixels.size(), run_passes, &rounds, job.node, job.node_index)
                  : run_passes(b.pixels, (uint32_t)pixels.size(), rd.first_sample, rd.sample_count, nullptr);
    if (st != PT_OK) return st;
    if (adaptive && group_count) HIP_TRY(ptk::launch_adaptive_finish_groups(stream, rd.width * rd.height, sc->adaptive.counts, job.d_group_films, group_count));
    if (adaptive && job.d_spectral)
        hipLaunchKernelGGL(k_adaptive_finish_spectral, dim3(sc->num_cus * 4), dim3(kBlock), 0, stream, rd.width * rd.height, job.spectral_bins, sc->adaptive.counts, job.d_spectral);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    auto t1 = std::chrono::steady_clock::now();
    clock.read(overlapped);
    if (profile) return read_profile(sc, plan, overlap, camera_rays, accumulated_pixels, clock, rounds, std::chrono::duration<double>(t1 - t0).count(), profile);
    return PT_OK;
}

pt_status probe_material(pt_scene* sc, int mode, uint32_t record, size_t n, const float* lambda, const float* a, size_t a_w, const float* b, size_t b_w,
                         float* f, float* wo, float* pdf) {
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf dl, da, db, df, dwo, dp;
    size_t m = n ? n : 1;
    HIP_TRY(dl.alloc(4 * m)); HIP_TRY(da.alloc(4 * m * 3)); HIP_TRY(db.alloc(4 * m * 3));
    HIP_TRY(df.alloc(4 * m)); HIP_TRY(dwo.alloc(4 * m * 3)); HIP_TRY(dp.alloc(4 * m));
    HIP_TRY(hipMemcpy(dl.p, lambda, 4 * n, hipMemcpyHostToDevice));
    if (a) HIP_TRY(hipMemcpy(da.p, a, 4 * n * a_w, hipMemcpyHostToDevice));
    if (b) HIP_TRY(hipMemcpy(db.p, b, 4 * n * b_w, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_material, dim3(256), dim3(kBlock), 0, 0, sc->d_blob, sc->d_tex, mode, record, (uint32_t)n, dl.as<float>(), da.as<float>(), db.as<float>(),
                       df.as<float>(), dwo.as<float>(), dp.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (f) HIP_TRY(hipMemcpy(f, df.p, 4 * n, hipMemcpyDeviceToHost));
    if (wo) HIP_TRY(hipMemcpy(wo, dwo.p, 4 * n * 3, hipMemcpyDeviceToHost));
    if (pdf) HIP_TRY(hipMemcpy(pdf, dp.p, 4 * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // namespace

extern "C" {

const char* pt_last_error(void) { return g_error.c_str(); }

const char* pt_device_info(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { g_device_info = "no HIP device"; return g_device_info.c_str(); }
    int dev = 0; hipGetDevice(&dev);
    hipDeviceProp_t p; hipGetDeviceProperties(&p, dev);
    char buf[256];
    snprintf(buf, sizeof(buf), "%s %s %d CUs, %.1f GB, LDS/block %zu KB", p.name, p.gcnArchName, p.multiProcessorCount,
             (double)p.totalGlobalMem / 1e9, p.sharedMemPerBlock / 1024);
    g_device_info = buf;
    return g_device_info.c_str();
}

// Device side of a scene: the blob and the texels on the current device, the staging mode, the kernels' LDS allowance.
static pt_status scene_to_device(pt_scene* sc) {
    hipError_t e = hipGetDevice(&sc->device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, sc->device);
    if (e != hipSuccess) return fail(PT_ERR_NO_DEVICE, hipGetErrorString(e));
    sc->num_cus = prop.multiProcessorCount;
    const pth::ScenePlan plan = pth::plan_scene(sc->tuning, sc->host.blob);   // (the tuning's edits of the blob, in place)
    sc->lacks = plan.lacks; sc->lds_mode = plan.lds_mode;
    sc->blob_words = (uint32_t)sc->host.blob.size();
    e = hipMalloc(&sc->d_blob, sizeof(uint32_t) * sc->host.blob.size());
    if (e == hipSuccess) e = hipMalloc(&sc->d_tex, sizeof(float) * (sc->host.tex.size() + 4));
    if (e == hipSuccess) e = hipMemcpy(sc->d_blob, sc->host.blob.data(), sizeof(uint32_t) * sc->host.blob.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sc->d_tex, sc->host.tex.data(), sizeof(float) * sc->host.tex.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, hipGetErrorString(e));
    if (sc->lds_mode != PT_LDS_NONE) {
        e = allow_lds_extend(kParkBlobLimitBytes);
        if (e == hipSuccess) e = allow_lds_shade(kLdsBlobLimitBytes > PT_SHADE_LDS_BUDGET ? kLdsBlobLimitBytes : PT_SHADE_LDS_BUDGET);   // (the FULL form's marginal tables ride behind the blob only within PT_SHADE_LDS_BUDGET)
        // (the parked light-sample kernels keep their waves' lists of live rays behind the blob: up to 16 waves x (64 L + 64) words)
        if (e == hipSuccess) e = allow_lds_shadow(kParkBlobLimitBytes + 16u * (64u * PT_MAX_LIGHT_SAMPLES + 64u) * 4u);
        if (e == hipSuccess) e = allow_lds_routed(kLdsBlobLimitBytes > PT_SHADE_LDS_BUDGET ? kLdsBlobLimitBytes : PT_SHADE_LDS_BUDGET, kLdsBlobLimitBytes);
        if (e != hipSuccess) return fail(PT_ERR_DEVICE, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
    }
    return PT_OK;
}

void pt_tuning_default(pt_tuning* t) {
    if (!t) return;
    memset(t, 0, sizeof(*t));
    const struct { const char* name; uint32_t bit; } flags[] = {
        {"PT_AMD_NO_LDS", PT_TUNE_NO_LDS}, {"PT_AMD_NO_CORE_LDS", PT_TUNE_NO_CORE_LDS}, {"PT_AMD_NO_PARK", PT_TUNE_NO_PARK},
#ifdef PT_EXPERIMENTS
        {"PT_AMD_POOL", PT_TUNE_EXPERIMENT_POOL},
#endif

        {"PT_AMD_EXACT_SLAB", PT_TUNE_EXACT_SLAB}, {"PT_AMD_NO_CULL", PT_TUNE_NO_CULL}, {"PT_AMD_NO_SWEEP", PT_TUNE_NO_SWEEP}, {"PT_AMD_NO_MESH_SWEEP", PT_TUNE_NO_MESH_SWEEP},
        {"PT_AMD_NO_KNOWN_LIGHT", PT_TUNE_NO_KNOWN_LIGHT}, {"PT_AMD_GENERAL_FORMS", PT_TUNE_GENERAL_FORMS}, {"PT_AMD_NO_FUSE", PT_TUNE_NO_FUSE}, {"PT_AMD_MULTI_RCCL", PT_TUNE_MULTI_RCCL}, {"PT_AMD_NO_AXIS_SCAN", PT_TUNE_NO_AXIS_SCAN}, {"PT_AMD_NO_ONE_LIGHT", PT_TUNE_NO_ONE_LIGHT}, {"PT_AMD_NO_CONVEX", PT_TUNE_NO_CONVEX}, {"PT_AMD_NO_MESH_SHORTCUTS", PT_TUNE_NO_MESH_SHORTCUTS},
        {"PT_AMD_NO_LIVE_LIST", PT_TUNE_NO_LIVE_LIST}, {"PT_AMD_NO_PASS_OVERLAP", PT_TUNE_NO_PASS_OVERLAP},
    };
    for (const auto& f : flags) if (env_u32(f.name, 0)) t->flags |= f.bit;
    if (env_u32("PT_AMD_STAGE_TIMING", 1) == 0) t->flags |= PT_TUNE_NO_STAGE_TIMING;
    t->batch_slots = env_u32("PT_AMD_BATCH", 0);
    t->blocks_per_cu = env_u32("PT_AMD_BLOCKS_PER_CU", 0);
    t->park_blocks_per_cu = env_u32("PT_AMD_PARK_BLOCKS_PER_CU", 0);
    t->park_dynamic = getenv("PT_AMD_PARK_DYNAMIC") && *getenv("PT_AMD_PARK_DYNAMIC") ? (env_u32("PT_AMD_PARK_DYNAMIC", 0) != 0 ? 1 : 0) : -1;
    t->shade_form = env_u32("PT_AMD_SHADE_FORM", 0);
    t->lds_all_limit = env_u32("PT_AMD_LDS_ALL_LIMIT", 0);
    t->multi_virtual = env_u32("PT_AMD_MULTI_VIRTUAL", 0);
    t->walk_evict_below = env_u32("PT_AMD_WALK_EVICT_BELOW", 0);
    t->walk_search_below = env_u32("PT_AMD_WALK_SEARCH_BELOW", 0);
    t->park_block = env_u32("PT_AMD_PARK_BLOCK", 0);
    t->light_prepass_max = env_u32("PT_AMD_LIGHT_PREPASS_MAX", 0);
    t->top_evict_below = env_u32("PT_AMD_TOP_EVICT_BELOW", 0);
    t->group_evict_below = env_u32("PT_AMD_GROUP_EVICT_BELOW", 0);
    t->flags |= (env_u32("PT_AMD_PASS_SKEW", 0) & PT_TUNE_PASS_SKEW_MASK) << PT_TUNE_PASS_SKEW_SHIFT;
}

pt_status pt_scene_create(const pt_scene_desc* desc, pt_scene** out) {
    pt_tuning t;
    pt_tuning_default(&t);   // the only place the PT_AMD_* environment is read
    return pt_scene_create_tuned(desc, &t, out);
}

pt_status pt_scene_create_tuned(const pt_scene_desc* desc, const pt_tuning* tuning, pt_scene** out) {
    if (!desc || !out || !tuning) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t r : tuning->reserved) if (r != 0) return fail(PT_ERR_INVALID_ARGUMENT, "pt_tuning::reserved must be 0");
    if (tuning->park_block != 0 && tuning->park_block != 256 && tuning->park_block != 512 && tuning->park_block != 1024)
        return fail(PT_ERR_INVALID_ARGUMENT, "pt_tuning::park_block (PT_AMD_PARK_BLOCK) must be 0, 256, 512 or 1024");
    if (tuning->shade_form > 2 || tuning->park_dynamic < -1 || tuning->park_dynamic > 1 || tuning->multi_virtual > 64 || tuning->walk_evict_below > 64 || tuning->walk_search_below > 64 || tuning->top_evict_below > 64 || tuning->group_evict_below > 64)
        return fail(PT_ERR_INVALID_ARGUMENT, "pt_tuning: shade_form in 0..2, park_dynamic in -1..1, multi_virtual, walk_evict_below, walk_search_below, top_evict_below, group_evict_below <= 64");
    // the tiled queue index (pt_stages.h qtile) multiplies in 32 bits: capacity <= 2^30; the grids are num_cus * blocks in an int
    if (tuning->batch_slots > (1u << 30) || tuning->blocks_per_cu > 1024u || tuning->park_blocks_per_cu > 1024u)
        return fail(PT_ERR_INVALID_ARGUMENT, "pt_tuning: batch_slots (PT_AMD_BATCH) <= 2^30, blocks_per_cu and park_blocks_per_cu <= 1024");
    pt_status st = ensure_device();
    if (st != PT_OK) return st;
    pt_scene* sc = new pt_scene();
    sc->tuning = *tuning;
    std::string err;
    if (!pth::build_host_scene(*desc, &sc->host, &err)) { delete sc; return fail(PT_ERR_INVALID_ARGUMENT, err); }
    st = scene_to_device(sc);
    if (st != PT_OK) { const std::string msg = g_error; pt_scene_destroy(sc); g_error = msg; return st; }
    *out = sc;
    return PT_OK;
}

static void multi_release(MultiSetup& m);
// a render entry starts (or is refused): whatever an earlier node render left is no longer described (pt_resident_assemble)
static void forget_node_render(pt_scene* sc) { if (sc) sc->multi.node_render = NodeRemembered(); }
// a group render of any kind starts (or a node one is refused): no group films, on one device or in shards, no denoised ones that came from them, no group bins
static void end_group_films(pt_scene* sc) {
    if (!sc) return;
    sc->groups_valid = false; sc->groups_denoised = false; sc->group_bins_valid = false;
    sc->group_shards.clear();
}
void pt_scene_destroy(pt_scene* sc) {
    if (!sc) return;
    for (pt_scene* r : sc->replicas) if (r) pt_scene_destroy(r);
    sc->replicas.clear();
    if (sc->multi.valid) multi_release(sc->multi);
    hipSetDevice(sc->device);
    sc->buf.release();
    sc->buf2.release();
    sc->adaptive.release();
    hipFree(sc->d_blob); hipFree(sc->d_tex);
    for (auto* list : {&sc->events, &sc->events2, &sc->pass_deps}) for (auto& e : *list) hipEventDestroy(e);
    if (sc->pass_stream) hipStreamDestroy(sc->pass_stream);
    delete sc;   // (the grow-only buffers go with it: the replicas are gone and the device is this scene's)
}

pt_status pt_render_device(pt_scene* sc, const pt_render_desc* rd, void* film_device, void* hip_stream, pt_profile* profile) {
    return render_impl(sc, rd, static_cast<float*>(film_device), static_cast<hipStream_t>(hip_stream), profile, RenderJob());
}

// What a render entry was called with, its arguments checked (rd, ad: normalised where the entry normalises them): the descs of the render and where its results go.
struct RenderCall {
    const pt_render_desc* rd = nullptr;
    const pt_adaptive_desc* ad = nullptr;   // the adaptive entries
    const pt_spectral_desc* sd = nullptr;   // the spectral entries
    float* film = nullptr;
    uint32_t* sample_counts = nullptr;      // the adaptive entries; stats: where the caller wants them
    double* stats = nullptr;
    float* spectral = nullptr;              // the spectral entries
    const pt_light_groups_desc* gd = nullptr;   // pt_render_light_groups; group_films: where the caller wants them (may be null)
    float* group_films = nullptr;
    bool passes = false;                    // pt_render_path_passes: no gd; group_films: where the caller wants the PT_PATH_PASSES pass films (may be null)
    const pt_path_expr_program* exprs = nullptr;   // pt_render_path_exprs: no gd; expr_groups: one light group id per instance of the scene, or null; group_films: where
    const uint8_t* expr_groups = nullptr;          // the caller wants the program's `outputs` expression films (may be null)
    bool group_bins = false;                // pt_render_light_groups_spectral (gd and sd): the group bins too; group_spectral: where the caller wants them (may be null)
    float* group_spectral = nullptr;
};

// The body of the five one-device entries: the device, the film and the planes kept with the scene, render_impl on the null stream, the read-backs and the resident
// spectral film and group films.  profile->seconds: render_impl's window for the fixed entries; for the adaptive ones the whole call.
static pt_status render_one(pt_scene* sc, const RenderCall& call, pt_profile* profile) {
    const pt_render_desc& rd = *call.rd;
    forget_node_render(sc);
    if (call.sd) { sc->spectral_valid = false; sc->spectral_shards.clear(); }   // (a spectral render starts: whatever the buffer held is no film from here on)
    const uint32_t films = call.passes ? (uint32_t)PT_PATH_PASSES : call.exprs ? call.exprs->outputs : call.gd ? call.gd->group_count : 0u;   // the resident group films this render leaves
    if (films) end_group_films(sc);   // (likewise the group films, the denoised ones that came from them, and the group bins)
    sc->groups_paired = false;   // (the resident film ends below)
    sc->resident.end();   // (film_cache and the adaptive buffers are written from here on; guides and denoised outputs belonged to the film before)
    HIP_TRY(hipSetDevice(sc->device));
    const size_t n_pixels = (size_t)rd.width * rd.height, film_bytes = sizeof(float) * 4 * n_pixels, spectral_bytes = call.sd ? sizeof(float) * call.sd->bins * n_pixels : 0;
    pt_status st = sc->film_cache.reserve(film_bytes);
    if (st == PT_OK && call.sd) st = sc->spectral_cache.reserve(spectral_bytes);
    const size_t group_bytes = film_bytes * films;
    if (st == PT_OK && films) st = sc->group_films_cache.reserve(group_bytes);
    if (st == PT_OK && call.gd) st = sc->group_table.reserve(call.gd->instance_count ? call.gd->instance_count : 1u);
    const size_t expr_table_bytes = sizeof(PxEntry) * PX_MAX_STATES, expr_instances = call.expr_groups ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u;
    if (st == PT_OK && call.exprs) st = sc->group_table.reserve(expr_table_bytes + (expr_instances ? expr_instances : 1u));   // (the table in front: 16-byte entries)
    if (st != PT_OK) return st;
    const size_t group_bins_bytes = call.group_bins ? spectral_bytes * call.gd->group_count : 0;
    const pt_status bins_reserved = call.group_bins ? sc->group_bins_cache.reserve(group_bins_bytes) : PT_OK;
    if (bins_reserved != PT_OK) (void)hipGetLastError();   // (the refused reservation is no error of a later launch: the scene stays usable)
    if (bins_reserved != PT_OK && bins_reserved != PT_ERR_OUT_OF_MEMORY) return bins_reserved;
    if (bins_reserved == PT_ERR_OUT_OF_MEMORY) {
        return fail(PT_ERR_OUT_OF_MEMORY, "the group bins need group_count x bins x width x height x 4 = " + std::to_string(call.gd->group_count) + " x " + std::to_string(call.sd->bins) +
                                              " x " + std::to_string(rd.width) + " x " + std::to_string(rd.height) + " x 4 = " + std::to_string(group_bins_bytes) +
                                              " bytes of device memory, which could not be reserved");
    }
    RenderJob job;
    job.adaptive = call.ad;
    LightGroupTable table{sc->group_table.as<uint8_t>(), call.gd ? call.gd->environment_group : 0u, call.gd ? call.gd->group_count : 0u};
    if (call.gd) {
        if (call.gd->instance_count) HIP_TRY(hipMemcpy(sc->group_table.p, call.gd->instance_group, call.gd->instance_count, hipMemcpyHostToDevice));
        job.groups = &table; job.d_group_films = sc->group_films_cache.as<float>();
    }
    if (call.passes) { job.classes = true; job.d_group_films = sc->group_films_cache.as<float>(); }
    if (call.exprs) {   // (the program's table, uploaded once per call: its `states` entries, the rest of the 64 zero — a state with no successor but 0 and no output)
        uint32_t entries[PX_MAX_STATES][4];
        memset(entries, 0, sizeof(entries));
        memcpy(entries, call.exprs->table, sizeof(uint32_t) * 4 * call.exprs->states);
        HIP_TRY(hipMemcpy(sc->group_table.p, entries, expr_table_bytes, hipMemcpyHostToDevice));
        if (expr_instances) HIP_TRY(hipMemcpy(sc->group_table.as<uint8_t>() + expr_table_bytes, call.expr_groups, expr_instances, hipMemcpyHostToDevice));
        job.exprs = call.exprs; job.d_expr_table = sc->group_table.as<PxEntry>();
        job.d_expr_groups = expr_instances ? sc->group_table.as<uint8_t>() + expr_table_bytes : nullptr;
        job.d_group_films = sc->group_films_cache.as<float>();
    }
    if (call.sd) { job.d_spectral = sc->spectral_cache.as<float>(); job.spectral_bins = call.sd->bins; }
    if (call.group_bins) job.d_group_bins = sc->group_bins_cache.as<float>();
    const hipStream_t stream = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    st = render_impl(sc, &rd, sc->film_cache.as<float>(), stream, profile, job);
    if (st != PT_OK) return st;
    HIP_TRY(hipMemcpy(call.film, sc->film_cache.p, film_bytes, hipMemcpyDeviceToHost));
    if (call.ad) {
        HIP_TRY(hipMemcpy(call.sample_counts, sc->adaptive.counts, sizeof(uint32_t) * n_pixels, hipMemcpyDeviceToHost));
        if (call.stats) HIP_TRY(hipMemcpy(call.stats, sc->adaptive.stats, sizeof(double) * 2 * n_pixels, hipMemcpyDeviceToHost));
    }
    if (call.sd && call.spectral) HIP_TRY(hipMemcpy(call.spectral, sc->spectral_cache.p, spectral_bytes, hipMemcpyDeviceToHost));
    if (call.group_bins && call.group_spectral) HIP_TRY(hipMemcpy(call.group_spectral, sc->group_bins_cache.p, group_bins_bytes, hipMemcpyDeviceToHost));
    if (call.group_bins) {
        sc->group_bins_width = rd.width; sc->group_bins_height = rd.height; sc->group_bins_groups = call.gd->group_count; sc->group_bins_bins = call.sd->bins;
        sc->group_bins_valid = true;
    }
    if (films && call.group_films) HIP_TRY(hipMemcpy(call.group_films, sc->group_films_cache.p, group_bytes, hipMemcpyDeviceToHost));
    if (films) { sc->groups_width = rd.width; sc->groups_height = rd.height; sc->groups_count = films; sc->groups_valid = true; }
    if (films && call.ad) sc->groups_paired = true;   // (the resident film set below and the group films came from this one render)
    if (call.ad && profile) profile->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();   // (the whole call: set-up, rounds, read-backs)
    if (call.sd) { sc->spectral_width = rd.width; sc->spectral_height = rd.height; sc->spectral_bins = call.sd->bins; sc->spectral_valid = true; }
    if (call.ad) {   // the resident set of include/pt_resident.h: film, counts and statistics, and the bins of a spectral render
        ResidentSet& r = sc->resident;
        r.parts = PT_RESIDENT_FILM | (call.sd ? PT_RESIDENT_BINS : 0u);
        r.width = rd.width; r.height = rd.height; r.bins = call.sd ? call.sd->bins : 0u;
        r.film = sc->film_cache.as<float>(); r.counts = sc->adaptive.counts; r.stats = sc->adaptive.stats; r.spectral = call.sd ? sc->spectral_cache.as<float>() : nullptr;
    }
    return PT_OK;
}

pt_status pt_render(pt_scene* sc, const pt_render_desc* rd, float* film, pt_profile* profile) {
    forget_node_render(sc);
    if (!sc || !rd || !film) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (rd->width == 0 || rd->height == 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    RenderCall call;
    call.rd = rd; call.film = film;
    return render_one(sc, call, profile);
}

pt_status pt_render_adaptive(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, float* film, uint32_t* sample_counts, double* stats,
                             pt_profile* profile) {
    forget_node_render(sc);
    if (!sc || !rdp || !adp || !film) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    pt_status st = pth::normalize_adaptive_desc(*rdp, *adp, sample_counts != nullptr, (uint32_t)sc->host.cameras.size(), &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.film = film; call.sample_counts = sample_counts; call.stats = stats;
    return render_one(sc, call, profile);
}

pt_status pt_render_spectral(pt_scene* sc, const pt_render_desc* rdp, const pt_spectral_desc* sdp, float* film, float* spectral, pt_profile* profile) {
    forget_node_render(sc);
    std::string err;
    pt_status st = pth::check_spectral_args(sc, rdp, sdp, film, spectral, &err);
    if (st != PT_OK) return fail(st, err);
    if (rdp->width == 0 || rdp->height == 0 || (uint64_t)rdp->width * rdp->height > 0xffffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and the film at most 2^32 - 1 pixels");
    RenderCall call;
    call.rd = rdp; call.sd = sdp; call.film = film; call.spectral = spectral;
    return render_one(sc, call, profile);
}

pt_status pt_render_adaptive_spectral(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_spectral_desc* sdp, float* film,
                                      uint32_t* sample_counts, double* stats, float* spectral, pt_profile* profile) {
    forget_node_render(sc);
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    pt_status st = pth::check_adaptive_spectral_args(sc, rdp, adp, sdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, film, sample_counts, spectral, &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.sd = sdp; call.film = film; call.sample_counts = sample_counts; call.stats = stats; call.spectral = spectral;
    return render_one(sc, call, profile);
}

pt_status pt_render_light_groups(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gdp, float* film, float* group_films, pt_profile* profile) {
    forget_node_render(sc);
    std::string err;
    const pt_status st = pth::check_light_groups_args(sc, rdp, gdp, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film, &err);
    if (st != PT_OK) return fail(st, err);
    if (rdp->width == 0 || rdp->height == 0 || (uint64_t)rdp->width * rdp->height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = rdp; call.gd = gdp; call.film = film; call.group_films = group_films;
    return render_one(sc, call, profile);
}

pt_status pt_render_adaptive_light_groups(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_light_groups_desc* gdp, float* film,
                                          uint32_t* sample_counts, double* stats, float* group_films, pt_profile* profile) {
    forget_node_render(sc);
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    const pt_status st = pth::check_adaptive_light_groups_args(sc, rdp, adp, gdp, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, sc ? (uint32_t)sc->host.cameras.size() : 0u,
                                                               film, sample_counts, &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    if ((uint64_t)rd.width * rd.height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.gd = gdp; call.film = film; call.sample_counts = sample_counts; call.stats = stats; call.group_films = group_films;
    return render_one(sc, call, profile);
}

// include/pt_light_groups.h, "Path passes": a group render of PT_PATH_PASSES films routed by the path's history; what it leaves is the scene's resident group films
pt_status pt_render_path_passes(pt_scene* sc, const pt_render_desc* rdp, const pt_path_passes_desc* pdp, float* film, float* pass_films, pt_profile* profile) {
    forget_node_render(sc);
    std::string err;
    const pt_status st = pth::check_path_passes_args(sc, rdp, pdp, film, &err);
    if (st != PT_OK) return fail(st, err);
    if (rdp->width == 0 || rdp->height == 0 || (uint64_t)rdp->width * rdp->height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = rdp; call.passes = true; call.film = film; call.group_films = pass_films;
    return render_one(sc, call, profile);
}

pt_status pt_render_adaptive_path_passes(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_path_passes_desc* pdp, float* film,
                                         uint32_t* sample_counts, double* stats, float* pass_films, pt_profile* profile) {
    forget_node_render(sc);
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    const pt_status st = pth::check_adaptive_path_passes_args(sc, rdp, adp, pdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, film, sample_counts, &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    if ((uint64_t)rd.width * rd.height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.passes = true; call.film = film; call.sample_counts = sample_counts; call.stats = stats; call.group_films = pass_films;
    return render_one(sc, call, profile);
}

// include/pt_light_groups.h, "Path expressions": a group render of program->outputs films routed by the program's automaton; what it leaves is the scene's resident
// group films
pt_status pt_render_path_exprs(pt_scene* sc, const pt_render_desc* rdp, const pt_path_expr_program* program, const uint8_t* instance_group, uint32_t n_instances, float* film,
                               float* expr_films, pt_profile* profile) {
    forget_node_render(sc);
    std::string err;
    const pt_status st = pth::check_path_exprs_args(sc, rdp, program, instance_group, n_instances, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film, &err);
    if (st != PT_OK) return fail(st, err);
    if (rdp->width == 0 || rdp->height == 0 || (uint64_t)rdp->width * rdp->height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = rdp; call.exprs = program; call.expr_groups = instance_group; call.film = film; call.group_films = expr_films;
    return render_one(sc, call, profile);
}

pt_status pt_render_adaptive_path_exprs(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_path_expr_program* program, const uint8_t* instance_group,
                                        uint32_t n_instances, float* film, uint32_t* sample_counts, double* stats, float* expr_films, pt_profile* profile) {
    forget_node_render(sc);
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    const pt_status st = pth::check_adaptive_path_exprs_args(sc, rdp, adp, program, instance_group, n_instances, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u,
                                                             sc ? (uint32_t)sc->host.cameras.size() : 0u, film, sample_counts, &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    if ((uint64_t)rd.width * rd.height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.exprs = program; call.expr_groups = instance_group; call.film = film; call.sample_counts = sample_counts; call.stats = stats;
    call.group_films = expr_films;
    return render_one(sc, call, profile);
}

// include/pt_light_groups_spectral.h: a group render with a spectral desc beside its groups desc — the total bins as pt_render_spectral makes them, and every
// group's own (k_accumulate_group_bins)
pt_status pt_render_light_groups_spectral(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gdp, const pt_spectral_desc* sdp, float* film,
                                          float* group_films, float* spectral, float* group_spectral, pt_profile* profile) {
    forget_node_render(sc);
    std::string err;
    const pt_status st = pth::check_light_groups_spectral_args(sc, rdp, gdp, sdp, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, film, &err);
    if (st != PT_OK) return fail(st, err);
    RenderCall call;
    call.rd = rdp; call.gd = gdp; call.sd = sdp; call.film = film; call.group_films = group_films; call.spectral = spectral;
    call.group_bins = true; call.group_spectral = group_spectral;
    return render_one(sc, call, profile);
}

pt_status pt_light_groups_spectral_resident(pt_scene* sc, uint32_t* width, uint32_t* height, uint32_t* group_count, uint32_t* bins) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!width || !height || !group_count || !bins) return fail(PT_ERR_INVALID_ARGUMENT, "width, height, group_count or bins is null");
    const bool v = sc->group_bins_valid;
    *width = v ? sc->group_bins_width : 0u; *height = v ? sc->group_bins_height : 0u; *group_count = v ? sc->group_bins_groups : 0u; *bins = v ? sc->group_bins_bins : 0u;
    return PT_OK;
}

// One launch over resident planes where they lie (defined beside run_resident_shards, its node form)
using ResidentLaunch = std::function<hipError_t(float* d_params, float* d_out, hipStream_t stream)>;
static pt_status apply_resident(pt_scene* sc, GrowBuf pt_scene::*cache, size_t cap_floats, const void* params, size_t param_bytes, void* out, size_t out_bytes,
                                const ResidentLaunch& launch, bool wait = true);

// pt_light_groups_relamp's kernel over group_bins_cache, on the stream the render ran on (the null stream): the matrix goes up, K planes come back
pt_status pt_light_groups_relamp_resident(pt_scene* sc, uint32_t K, const float* matrix, float* out) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "the re-lamped planes (out) are null");
    if (!sc->group_bins_valid) return fail(PT_ERR_INVALID_ARGUMENT, "the scene has no resident group bins: pt_render_light_groups_spectral must have succeeded on it");
    std::string err;
    const pt_status st = pth::check_relamp_matrix(K, sc->group_bins_groups, sc->group_bins_bins, matrix, &err);
    if (st != PT_OK) return fail(st, err);
    HIP_TRY(hipSetDevice(sc->device));
    const uint32_t planes = sc->group_bins_groups * sc->group_bins_bins;
    const size_t n_pixels = (size_t)sc->group_bins_width * sc->group_bins_height;
    const size_t matrix_floats = (size_t)PT_SPECTRAL_MAX_RESPONSES * PT_LIGHT_GROUPS_MAX * PT_SPECTRAL_MAX_BINS;
    return apply_resident(sc, &pt_scene::relamp_cache, matrix_floats, matrix, sizeof(float) * K * planes, out, sizeof(float) * K * n_pixels,
                          [&](float* d_matrix, float* d_out, hipStream_t stream) {
                              return ptk::launch_light_groups_relamp(ptk::spectral_project_grid(sc->num_cus, (uint32_t)n_pixels), stream, (uint32_t)n_pixels, planes, K, d_matrix,
                                                                     sc->group_bins_cache.as<float>(), d_out);
                          });
}

pt_status pt_light_groups_resident(pt_scene* sc, uint32_t* width, uint32_t* height, uint32_t* group_count) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!width || !height || !group_count) return fail(PT_ERR_INVALID_ARGUMENT, "width, height or group_count is null");
    *width = sc->groups_valid ? sc->groups_width : 0u; *height = sc->groups_valid ? sc->groups_height : 0u; *group_count = sc->groups_valid ? sc->groups_count : 0u;
    return PT_OK;
}

// include/pt_light_groups.h: pt_light_groups_mix's kernel over group_films_cache, on the stream the render ran on (the null stream), so the group films never cross the bus.
// (`films`: group_films_cache, or the denoised group films of include/pt_light_groups_denoise.h — the same size and count)
static pt_status mix_resident_films(pt_scene* sc, const float* films, const float* matrices, float* out);
static pt_status mix_resident_node(pt_scene* sc, const float* matrices, float* out);
pt_status pt_light_groups_mix_resident(pt_scene* sc, const float* matrices, float* out) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "out_xyzw is null");
    if (!sc->groups_valid) return fail(PT_ERR_INVALID_ARGUMENT, "the scene has no resident group films: pt_render_light_groups must have succeeded on it");
    if (!sc->group_shards.empty()) return mix_resident_node(sc, matrices, out);
    return mix_resident_films(sc, sc->group_films_cache.as<float>(), matrices, out);
}
pt_status pt_light_groups_mix_resident_denoised(pt_scene* sc, const float* matrices, float* out) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "out_xyzw is null");
    if (!sc->groups_denoised) return fail(PT_ERR_INVALID_ARGUMENT, "the scene has no resident denoised group films: pt_denoise_light_groups_resident must have succeeded on it");
    return mix_resident_films(sc, sc->group_den_films.as<float>(), matrices, out);
}
pt_status pt_light_groups_denoised_resident(pt_scene* sc, uint32_t* width, uint32_t* height, uint32_t* group_count) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!width || !height || !group_count) return fail(PT_ERR_INVALID_ARGUMENT, "width, height or group_count is null");
    *width = sc->groups_denoised ? sc->groups_width : 0u; *height = sc->groups_denoised ? sc->groups_height : 0u; *group_count = sc->groups_denoised ? sc->groups_count : 0u;
    return PT_OK;
}
static pt_status mix_resident_films(pt_scene* sc, const float* films, const float* matrices, float* out) {
    std::string err;
    const pt_status st = pth::check_light_groups_matrices(sc->groups_count, matrices, &err);
    if (st != PT_OK) return fail(st, err);
    HIP_TRY(hipSetDevice(sc->device));
    const size_t n_pixels = (size_t)sc->groups_width * sc->groups_height, matrix_floats = (size_t)PT_LIGHT_GROUPS_MAX * 12;   // (the film behind them stays 16-byte aligned)
    return apply_resident(sc, &pt_scene::group_mix_cache, matrix_floats, matrices, sizeof(float) * 9 * sc->groups_count, out, sizeof(float) * 4 * n_pixels,
                          [&](float* d_matrices, float* d_out, hipStream_t stream) {
                              return ptk::launch_light_groups_mix(stream, (uint32_t)n_pixels, sc->groups_count, films, d_matrices, d_out);
                          });
}

pt_status pt_spectral_resident(pt_scene* sc, uint32_t* width, uint32_t* height, uint32_t* bins) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!width || !height || !bins) return fail(PT_ERR_INVALID_ARGUMENT, "width, height or bins is null");
    *width = sc->spectral_valid ? sc->spectral_width : 0u; *height = sc->spectral_valid ? sc->spectral_height : 0u; *bins = sc->spectral_valid ? sc->spectral_bins : 0u;
    return PT_OK;
}

static pt_status project_resident_node(pt_scene* sc, uint32_t K, const float* matrix, float* out);
static pt_status project_device_bins(pt_scene* sc, uint32_t K, const float* matrix, uint32_t bins, size_t n_pixels, const float* d_bins, float* out);

// include/pt_spectral.h: pt_spectral_project's kernel over spectral_cache, on the stream the render ran on (the null stream), so the bins never cross the bus.
pt_status pt_spectral_project_resident(pt_scene* sc, uint32_t K, const float* matrix, float* out) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "the developed planes (out) are null");
    if (!sc->spectral_valid) return fail(PT_ERR_INVALID_ARGUMENT, "the scene has no resident spectral film: pt_render_spectral or pt_render_adaptive_spectral must have succeeded on it");
    std::string err;
    const pt_status st = pth::check_spectral_matrix(K, sc->spectral_bins, matrix, &err);
    if (st != PT_OK) return fail(st, err);
    if (!sc->spectral_shards.empty()) return project_resident_node(sc, K, matrix, out);
    return project_device_bins(sc, K, matrix, sc->spectral_bins, (size_t)sc->spectral_width * sc->spectral_height, sc->spectral_cache.as<float>(), out);
}
// pt_spectral_project's kernel over `bins` planes of n_pixels on the scene's device: the matrix goes up, K planes come back
static pt_status project_device_bins(pt_scene* sc, uint32_t K, const float* matrix, uint32_t bins, size_t n_pixels, const float* d_bins, float* out) {
    HIP_TRY(hipSetDevice(sc->device));
    return apply_resident(sc, &pt_scene::project_cache, (size_t)PT_SPECTRAL_MAX_RESPONSES * PT_SPECTRAL_MAX_BINS, matrix, sizeof(float) * K * bins, out,
                          sizeof(float) * K * n_pixels, [&](float* d_matrix, float* d_out, hipStream_t stream) {
                              return ptk::launch_spectral_project(ptk::spectral_project_grid(sc->num_cus, (uint32_t)n_pixels), stream, (uint32_t)n_pixels, bins, K, d_matrix, d_bins, d_out);
                          });
}

uint32_t pt_device_count(void) {
    int n = 0;
    return (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? (uint32_t)n : 0u;
}

extern "C++" {   // (C++ helpers inside the extern "C" region of the API functions)
// RCCL, bound on first use: a single-process render pays nothing for it, and the library loads on machines without it.
namespace {
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclReduce) reduce = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    bool ok() const { return comm_init_all && comm_destroy && reduce && all_reduce && group_start && group_end && error_string; }
};
Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { r.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (r.handle) break; }
        if (!r.handle) return;
        r.comm_init_all = reinterpret_cast<decltype(r.comm_init_all)>(dlsym(r.handle, "ncclCommInitAll"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(r.handle, "ncclCommDestroy"));
        r.reduce = reinterpret_cast<decltype(r.reduce)>(dlsym(r.handle, "ncclReduce"));
        r.all_reduce = reinterpret_cast<decltype(r.all_reduce)>(dlsym(r.handle, "ncclAllReduce"));
        r.group_start = reinterpret_cast<decltype(r.group_start)>(dlsym(r.handle, "ncclGroupStart"));
        r.group_end = reinterpret_cast<decltype(r.group_end)>(dlsym(r.handle, "ncclGroupEnd"));
        r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(r.handle, "ncclGetErrorString"));
    });
    return r;
}
}  // namespace
}  // extern "C++"

// dst += src over n float4 pixels: the films of the virtual devices that share one physical device (pt_tuning::multi_virtual)
__global__ void __launch_bounds__(kBlock) k_film_add(float4* __restrict__ dst, const float4* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 a = dst[i], b = src[i];
        dst[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}
// dst += src over n counts / n statistics: pt_render_adaptive_multi's sample counts and (S1, S2) of those virtual devices (0 outside a device's shard)
__global__ void __launch_bounds__(kBlock) k_u32_add(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = dst[i] + src[i];
}
__global__ void __launch_bounds__(kBlock) k_f64_add(double* __restrict__ dst, const double* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = dst[i] + src[i];
}

static void multi_release(MultiSetup& m) {
    for (size_t v = 0; v < m.films.size(); ++v) {
        if (m.devices.empty()) break;
        hipSetDevice(m.devices[v / m.virt]);
        if (v < m.streams.size() && m.streams[v]) hipStreamDestroy(m.streams[v]);
        if (m.films[v]) hipFree(m.films[v]);
    }
    for (size_t p = 0; p < m.comms.size(); ++p) if (m.comms[p]) { hipSetDevice(m.devices[p]); rccl().comm_destroy(m.comms[p]); }
    m = MultiSetup();   // (the staging buffers go with it)
}

// Streams, device films and (for more than one physical device) the RCCL communicator of a device set, made once per scene and film size.
static pt_status multi_setup(pt_scene* sc, const std::vector<int>& devices, uint32_t virt, bool use_rccl, size_t film_bytes) {
    MultiSetup& m = sc->multi;
    if (m.valid && m.devices == devices && m.virt == virt && m.rccl == use_rccl && m.film_bytes >= film_bytes) return PT_OK;
    multi_release(m);
    m.devices = devices; m.virt = virt; m.rccl = use_rccl; m.film_bytes = film_bytes;
    const size_t nv = devices.size() * virt;
    m.films.assign(nv, nullptr); m.streams.assign(nv, nullptr);
    m.staging = std::vector<GrowBuf>(nv);
    for (GrowBuf& h : m.staging) h.pinned = true;
    for (size_t v = 0; v < nv; ++v) {
        hipError_t e = hipSetDevice(devices[v / virt]);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&m.streams[v], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc(&m.films[v], film_bytes);
        if (e != hipSuccess) { multi_release(m); return fail(e == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string("pt_render_multi set-up: ") + hipGetErrorString(e)); }
    }
    if (use_rccl) {
        if (!rccl().ok()) { multi_release(m); return fail(PT_ERR_DEVICE, "librccl.so could not be loaded: pt_render_multi needs RCCL for more than one device"); }
        m.comms.assign(devices.size(), nullptr);
        ncclResult_t rc = rccl().comm_init_all(m.comms.data(), (int)devices.size(), devices.data());
        if (rc != ncclSuccess) { multi_release(m); return fail(PT_ERR_DEVICE, std::string("ncclCommInitAll: ") + rccl().error_string(rc)); }
    }
    m.valid = true;
    return PT_OK;
}

// The devices of a node call (pt_render_multi, pt_render_adaptive_multi): the physical devices of the mask, the virtual devices per physical one
// (pt_tuning::multi_virtual, a test mode), n = shards = host threads = streams = replicas, and whether the exchange between physical devices takes RCCL
// (always for more than one; PT_TUNE_MULTI_RCCL takes it even for one: the call path of a node, on a single GPU).
struct Node {
    std::vector<int> devices;
    uint32_t virt = 1;
    int np = 0, n = 0;
    bool use_rccl = false;
    std::vector<pt_scene*> scene_of;   // per virtual device: this scene or its replica
    bool single(const pt_scene* sc) const { return !use_rccl && n == 1 && devices[0] == sc->device; }   // (the one-device call itself)
};
static pt_status node_devices(pt_scene* sc, uint64_t device_mask, Node* node) {
    const uint32_t visible = pt_device_count();
    if (visible == 0) return no_device();
    for (uint32_t d = 0; d < visible && d < 64; ++d) if (device_mask == 0 || ((device_mask >> d) & 1ull)) node->devices.push_back((int)d);
    if (node->devices.empty()) return fail(PT_ERR_INVALID_ARGUMENT, "device_mask names no visible HIP device");
    node->np = (int)node->devices.size();
    node->virt = sc->tuning.multi_virtual > 1 ? sc->tuning.multi_virtual : 1u;
    node->n = node->np * (int)node->virt;
    node->use_rccl = node->np > 1 || (sc->tuning.flags & PT_TUNE_MULTI_RCCL) != 0;
    return PT_OK;
}
// one replica per (virtual) device — this scene itself for the first one on its own device — made on first use and kept on the scene; then the
// streams, device films and communicator (multi_setup)
static pt_status node_prepare(pt_scene* sc, Node& node, size_t film_bytes) {
    const uint32_t visible = pt_device_count(), virt = node.virt;
    if (sc->replicas.size() < (size_t)visible * virt) sc->replicas.resize((size_t)visible * virt, nullptr);
    node.scene_of.assign(node.n, nullptr);
    for (int v = 0; v < node.n; ++v) {
        const int d = node.devices[v / virt];
        const size_t slot = (size_t)d * virt + (size_t)v % virt;
        if (d == sc->device && v % (int)virt == 0) { node.scene_of[v] = sc; continue; }
        if (!sc->replicas[slot]) {
            HIP_TRY(hipSetDevice(d));
            pt_scene* r = new pt_scene();
            r->host = sc->host;
            r->tuning = sc->tuning;
            pt_status st = scene_to_device(r);
            if (st != PT_OK) { const std::string msg = g_error; pt_scene_destroy(r); g_error = msg; return st; }
            sc->replicas[slot] = r;
        }
        node.scene_of[v] = sc->replicas[slot];
    }
    return multi_setup(sc, node.devices, virt, node.use_rccl, film_bytes);
}
// worker(v) for every virtual device: one host thread each, v = 0 on the calling thread
static void node_run(int n, const std::function<void(int)>& worker) {
    std::vector<std::thread> pool;
    for (int v = 1; v < n; ++v) pool.emplace_back(worker, v);
    worker(0);
    for (auto& t : pool) t.join();
}
// The gather of per-device buffers into the first device of the mask: (1) the virtual devices of one physical device added on that device (their
// streams are synchronised), (2) one grouped ncclReduce(sum) per buffer between the physical devices, over xGMI.  Every device's buffers are zero outside
// its own tiles, so the sums are gathers and keep every bit.
struct GatherPart { std::vector<void*> bufs; size_t count; ncclDataType_t type; };   // bufs: per virtual device; count: elements (floats, u32, f64)
static pt_status node_gather(MultiSetup& m, const Node& node, const std::vector<GatherPart>& parts) {
    const uint32_t virt = node.virt;
    for (int p = 0; p < node.np && virt > 1; ++p) {
        HIP_TRY(hipSetDevice(node.devices[p]));
        hipStream_t s = m.streams[(size_t)p * virt];
        for (const GatherPart& g : parts)
            for (uint32_t j = 1; j < virt; ++j) {
                void *dst = g.bufs[(size_t)p * virt], *src = g.bufs[(size_t)p * virt + j];
                if (g.type == ncclFloat) hipLaunchKernelGGL(k_film_add, dim3(1024), dim3(kBlock), 0, s, static_cast<float4*>(dst), static_cast<const float4*>(src), g.count / 4);
                else if (g.type == ncclUint32) hipLaunchKernelGGL(k_u32_add, dim3(1024), dim3(kBlock), 0, s, static_cast<uint32_t*>(dst), static_cast<const uint32_t*>(src), g.count);
                else hipLaunchKernelGGL(k_f64_add, dim3(1024), dim3(kBlock), 0, s, static_cast<double*>(dst), static_cast<const double*>(src), g.count);
            }
        HIP_TRY(hipGetLastError());
        if (!node.use_rccl) HIP_TRY(hipStreamSynchronize(s));
    }
    if (node.use_rccl) {
        ncclResult_t rc = rccl().group_start();
        for (int p = 0; p < node.np && rc == ncclSuccess; ++p) {
            hipSetDevice(node.devices[p]);
            for (const GatherPart& g : parts) {
                void* b = g.bufs[(size_t)p * virt];
                rc = rccl().reduce(b, b, g.count, g.type, ncclSum, 0, m.comms[p], m.streams[(size_t)p * virt]);
                if (rc != ncclSuccess) break;
            }
        }
        ncclResult_t rc2 = rccl().group_end();
        if (rc == ncclSuccess) rc = rc2;
        if (rc != ncclSuccess) { multi_release(m); return fail(PT_ERR_DEVICE, std::string("ncclReduce: ") + rccl().error_string(rc)); }
        for (int p = 0; p < node.np; ++p) { hipSetDevice(node.devices[p]); if (hipStreamSynchronize(m.streams[(size_t)p * virt]) != hipSuccess) { multi_release(m); return fail(PT_ERR_DEVICE, "stream synchronisation after the film reduce failed"); } }
    }
    return PT_OK;
}
// the summed ray counters and stage figures of the workers' profiles
static void node_profile(const std::vector<pt_profile>& profiles, pt_profile* profile) {
    memset(profile, 0, sizeof(*profile));
    for (const pt_profile& p : profiles) {
        profile->bounce_rays += p.bounce_rays; profile->shadow_rays += p.shadow_rays; profile->light_rays += p.light_rays;
        profile->camera_rays += p.camera_rays; profile->env_hits += p.env_hits;
        for (int k = 0; k < 5; ++k) { profile->kernel_seconds[k] += p.kernel_seconds[k]; profile->kernel_launches[k] += p.kernel_launches[k]; profile->stage_items[k] += p.stage_items[k]; }
        profile->stage_items[5] += p.stage_items[5];
    }
}
// whatever happens in a node call, the caller gets its current device back
struct DeviceGuard {
    int d = 0;
    bool ok = false;
    DeviceGuard() { ok = hipGetDevice(&d) == hipSuccess; }
    ~DeviceGuard() { if (ok) hipSetDevice(d); }
};
static std::string device_name(const Node& node, int v) {
    return "device " + std::to_string(node.devices[v / node.virt]) + (node.virt > 1 ? "." + std::to_string(v % node.virt) : "");
}

// The per-pixel payload of a node call beside its film: the bins of a spectral call (pt_render_spectral_multi, pt_render_adaptive_spectral_multi; DESIGN.md
// section 14) or the group films of a group call (pt_render_light_groups_multi, pt_render_adaptive_light_groups_multi; DESIGN.md section 15 "On every device
// of a node").  It is never reduced: every device packs the planes of its own tiles (k_spectral_pack, k_light_groups_pack), copies them to its pinned
// staging buffer and its host thread scatters them into the caller's array; the packed planes stay on the device as its part of the scene's resident film
// or group films.
struct NodePayload {
    const ShardKind* kind = nullptr;
    uint32_t planes = 0;           // bins, or groups
    size_t film_pixels = 0;
    float* host = nullptr;         // the caller's planes (null, a group call's choice: nothing is copied to the host)
    std::vector<double> seconds;   // per worker: its pack, copy and scatter
};
// Part of the set-up: every device's pixel list (kept on its scene), full-size planes, packed planes and — with a host array — staging buffer, made once per
// size and kept.  A shard without a pixel gets no packed buffer.  rd: normalised.
static pt_status node_prepare_payload(MultiSetup& m, const Node& node, const pt_render_desc& rd, const ShardKind& kind, uint32_t planes, float* host, NodePayload* np) {
    np->kind = &kind; np->planes = planes; np->film_pixels = (size_t)rd.width * rd.height; np->host = host; np->seconds.assign(node.n, 0.0);
    for (int v = 0; v < node.n; ++v) {
        pt_scene* s = node.scene_of[v];
        Shard& shard = s->*kind.shard;
        shard.px = pth::shard_pixels(rd.width, rd.height, rd.tile_width, rd.tile_height, node.n > 1 ? (uint32_t)v : 0u, node.n > 1 ? (uint32_t)node.n : 0u);
        HIP_TRY(hipSetDevice(node.devices[v / node.virt]));
        const size_t elem_bytes = sizeof(float) * kind.floats, packed_bytes = elem_bytes * planes * shard.px.size();
        pt_status st = (s->*kind.full).reserve(elem_bytes * planes * np->film_pixels);
        if (st == PT_OK) st = shard.packed.reserve(packed_bytes);
        if (st == PT_OK && host) st = m.staging[v].reserve(packed_bytes);
        if (st != PT_OK) return st;
    }
    return PT_OK;
}
// Worker v behind its render (the stream is idle: render_impl synchronised it): pack by the list render_impl left in buf.pixels, copy, scatter.  The shards
// are disjoint and cover the film (every pixel is in exactly one list: tests/test_spectral_multi.py, tests/test_light_groups_multi.py), so the threads never
// write the same element and the caller's array needs no zeroing.  Without a host array the pack still runs: the packed shard is what stays resident.
static pt_status node_payload_exchange(MultiSetup& m, const Node& node, NodePayload& np, int v) {
    pt_scene* s = node.scene_of[v];
    const ShardKind& kind = *np.kind;
    const Shard& shard = s->*kind.shard;
    const uint32_t n_own = (uint32_t)shard.px.size();
    if (n_own == 0) return PT_OK;
    const auto t = std::chrono::steady_clock::now();
    HIP_TRY(ptk::launch_shard_pack(kind.floats, ptk::shard_pack_grid(s->num_cus, n_own), m.streams[v], (s->*kind.full).as<float>(), (uint32_t)np.film_pixels, s->buf.pixels, n_own,
                                   np.planes, shard.packed.as<float>()));
    if (np.host) HIP_TRY(hipMemcpyAsync(m.staging[v].p, shard.packed.p, sizeof(float) * kind.floats * np.planes * n_own, hipMemcpyDeviceToHost, m.streams[v]));
    HIP_TRY(hipStreamSynchronize(m.streams[v]));
    if (np.host) shard_scatter_host(kind, m.staging[v].p, shard.px, np.planes, np.host, np.film_pixels);
    np.seconds[v] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
    return PT_OK;
}
static double node_payload_seconds(const NodePayload& np) { return np.seconds.empty() ? 0.0 : *std::max_element(np.seconds.begin(), np.seconds.end()); }

// A kernel over node-resident shards where they lie: `matrix_bytes` of `matrix` to every device that holds a shard of `shards`, into the scene's `cache` (the
// matrix at its cap size, matrix_floats, then the output); `launch(s, n_own, d_matrix, packed, d_out)` over the shard's packed planes (plane stride n_own);
// out_planes * n_own elements of `kind` back per device, scattered into `out` by the rule the shards were scattered by.
// A kernel over resident planes where they lie, on the stream they were made on (the null stream) of the scene's device, which is current: `param_bytes` of
// `params` up into the scene's `cache` — the parameter block at its cap size, cap_floats, then the output —, `launch(d_params, d_out, stream)`, and out_bytes
// of the output back into `out`.  wait false: nothing is synchronised (run_resident_shards enqueues on every device first).
static pt_status apply_resident(pt_scene* sc, GrowBuf pt_scene::*cache, size_t cap_floats, const void* params, size_t param_bytes, void* out, size_t out_bytes,
                                const ResidentLaunch& launch, bool wait) {
    const pt_status cached = (sc->*cache).reserve(sizeof(float) * cap_floats + out_bytes);
    if (cached != PT_OK) return cached;
    float* d_params = (sc->*cache).as<float>();
    float* d_out = d_params + cap_floats;
    const hipStream_t stream = nullptr;
    HIP_TRY(hipMemcpyAsync(d_params, params, param_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(launch(d_params, d_out, stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream));
    if (wait) HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}
using ShardLaunch = std::function<hipError_t(pt_scene* s, uint32_t n_own, const float* d_matrix, const float* packed, float* d_out)>;
static pt_status run_resident_shards(const std::vector<pt_scene*>& shards, const ShardKind& kind, uint32_t out_planes, size_t film_pixels, const float* matrix,
                                     size_t matrix_bytes, size_t matrix_floats, GrowBuf pt_scene::*cache, float* out, const ShardLaunch& launch) {
    DeviceGuard guard;
    std::vector<std::vector<float>> back(shards.size());
    for (size_t v = 0; v < shards.size(); ++v) {
        pt_scene* s = shards[v];
        const Shard& shard = s->*kind.shard;
        const uint32_t n_own = (uint32_t)shard.px.size();
        if (n_own == 0) continue;
        HIP_TRY(hipSetDevice(s->device));
        back[v].resize((size_t)kind.floats * out_planes * n_own);
        const pt_status st = apply_resident(s, cache, matrix_floats, matrix, matrix_bytes, back[v].data(), sizeof(float) * back[v].size(),
                                            [&](float* d_matrix, float* d_out, hipStream_t) { return launch(s, n_own, d_matrix, shard.packed.as<float>(), d_out); }, false);
        if (st != PT_OK) return st;
    }
    for (size_t v = 0; v < shards.size(); ++v) {
        pt_scene* s = shards[v];
        const Shard& shard = s->*kind.shard;
        if (shard.px.empty()) continue;
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamSynchronize(nullptr));
        shard_scatter_host(kind, back[v].data(), shard.px, out_planes, out, film_pixels);
    }
    return PT_OK;
}
// pt_spectral_project_resident of a node-resident film: pt_spectral_project's kernel over every shard's packed bins, K planes of floats back.
static pt_status project_resident_node(pt_scene* sc, uint32_t K, const float* matrix, float* out) {
    const uint32_t bins = sc->spectral_bins;
    return run_resident_shards(sc->spectral_shards, kSpectralShard, K, (size_t)sc->spectral_width * sc->spectral_height, matrix, sizeof(float) * K * bins,
                               (size_t)PT_SPECTRAL_MAX_RESPONSES * PT_SPECTRAL_MAX_BINS, &pt_scene::project_cache, out,
                               [&](pt_scene* s, uint32_t n_own, const float* d_matrix, const float* packed, float* d_out) {
                                   return ptk::launch_spectral_project(ptk::spectral_project_grid(s->num_cus, n_own), nullptr, n_own, bins, K, d_matrix, packed, d_out);
                               });
}
// pt_light_groups_mix_resident of node-resident group films: pt_light_groups_mix's kernel over every shard's packed films, one film of pixels back.
static pt_status mix_resident_node(pt_scene* sc, const float* matrices, float* out) {
    std::string err;
    const pt_status checked = pth::check_light_groups_matrices(sc->groups_count, matrices, &err);
    if (checked != PT_OK) return fail(checked, err);
    const uint32_t groups = sc->groups_count;
    return run_resident_shards(sc->group_shards, kGroupShard, 1u, (size_t)sc->groups_width * sc->groups_height, matrices, sizeof(float) * 9 * groups,
                               (size_t)PT_LIGHT_GROUPS_MAX * 12 /* (the film behind them stays 16-byte aligned) */, &pt_scene::group_mix_cache, out,
                               [&](pt_scene*, uint32_t n_own, const float* d_matrices, const float* packed, float* d_out) {
                                   return ptk::launch_light_groups_mix(nullptr, n_own, groups, packed, d_matrices, d_out);
                               });
}

// The node driver behind the six node entries (call: as for render_one): one worker per (virtual) device renders its shard of the film, the films are gathered
// on the first device of the mask and read back from there.  An adaptive call (pt_render_adaptive_multi) runs its rounds in lockstep over the NodeRounds and
// gathers counts and statistics too; a spectral call hands every worker's bins over by node_payload_exchange and leaves the packed shards resident; a group
// call does the same with every worker's group films.
static pt_status render_node(pt_scene* sc, const RenderCall& call, uint64_t device_mask, pt_profile* profile) {
    const pt_render_desc& rd = *call.rd;
    const bool adaptive = call.ad != nullptr;
    forget_node_render(sc);
    Node node;
    pt_status st = node_devices(sc, device_mask, &node);
    if (st != PT_OK) return st;
    if (node.single(sc)) return render_one(sc, call, profile);   // (the one-device entry's body: its checks are among this call's, and have passed)
    sc->groups_paired = false;
    sc->resident.end();   // (the shards of a node render are no film one device can filter until pt_resident_assemble is asked: include/pt_resident.h)

    DeviceGuard guard;
    const auto t_entry = std::chrono::steady_clock::now();
    const size_t pixels = (size_t)rd.width * rd.height, bytes = sizeof(float) * 4 * pixels;
    st = node_prepare(sc, node, bytes);
    if (st != PT_OK) return st;
    MultiSetup& m = sc->multi;
    const int n = node.n;
    const uint32_t virt = node.virt;
    for (int v = 0; v < n && adaptive; ++v) {   // (the adaptive buffers exist before the workers start: the exchange reads every device's image)
        HIP_TRY(hipSetDevice(node.devices[v / virt]));
        st = ensure_adaptive_buffers(node.scene_of[v], pixels);
        if (st != PT_OK) return st;
    }
    NodePayload ns, ng;   // (no node entry has both today)
    if (call.sd) {
        st = node_prepare_payload(m, node, rd, kSpectralShard, call.sd->bins, call.spectral, &ns);
        if (st != PT_OK) return st;
    }
    if (call.gd) {
        st = node_prepare_payload(m, node, rd, kGroupShard, call.gd->group_count, call.group_films, &ng);
        for (int v = 0; v < n && st == PT_OK; ++v) {   // (the group table's bytes on every device)
            pt_scene* s = node.scene_of[v];
            HIP_TRY(hipSetDevice(node.devices[v / virt]));
            st = s->group_table.reserve(call.gd->instance_count ? call.gd->instance_count : 1u);
            if (st == PT_OK && call.gd->instance_count) HIP_TRY(hipMemcpy(s->group_table.p, call.gd->instance_group, call.gd->instance_count, hipMemcpyHostToDevice));
        }
        if (st != PT_OK) return st;
    }
    NodeRounds nr;
    if (adaptive) {
        nr.lock.parties = n;
        nr.next.assign(n, 0u);
        for (int v = 0; v < n; ++v) nr.images.push_back(node.scene_of[v]->adaptive.unconverged);
        for (int v = 0; v < n; ++v) nr.merged.push_back(nr.images[(size_t)(v / (int)virt) * virt]);
        // the exchange of a round (run by the last worker to arrive): the images of the virtual devices ORed on their physical device, then one grouped
        // all-reduce (max = OR: the shards are disjoint) between the physical devices; every first virtual device then holds the film-wide image
        nr.exchange = [&]() -> pt_status {
            const auto t = std::chrono::steady_clock::now();
            int here = 0;
            HIP_TRY(hipGetDevice(&here));
            const unsigned blocks = (unsigned)std::min<size_t>(1024, std::max<size_t>(1, (pixels / 16 + kBlock - 1) / kBlock));
            for (int p = 0; p < node.np && virt > 1; ++p) {
                HIP_TRY(hipSetDevice(node.devices[p]));
                for (uint32_t j = 1; j < virt; ++j)
                    hipLaunchKernelGGL(k_mask_or, dim3(blocks), dim3(kBlock), 0, m.streams[(size_t)p * virt], nr.images[(size_t)p * virt], nr.images[(size_t)p * virt + j], pixels);
                HIP_TRY(hipGetLastError());
            }
            if (node.use_rccl) {
                ncclResult_t rc = rccl().group_start();
                for (int p = 0; p < node.np && rc == ncclSuccess; ++p) {
                    hipSetDevice(node.devices[p]);
                    uint8_t* img = nr.images[(size_t)p * virt];
                    rc = rccl().all_reduce(img, img, pixels, ncclUint8, ncclMax, m.comms[p], m.streams[(size_t)p * virt]);
                }
                ncclResult_t rc2 = rccl().group_end();
                if (rc == ncclSuccess) rc = rc2;
                if (rc != ncclSuccess) { hipSetDevice(here); return fail(PT_ERR_DEVICE, std::string("ncclAllReduce: ") + rccl().error_string(rc)); }
            }
            for (int p = 0; p < node.np; ++p) {
                HIP_TRY(hipSetDevice(node.devices[p]));
                HIP_TRY(hipStreamSynchronize(m.streams[(size_t)p * virt]));
            }
            HIP_TRY(hipSetDevice(here));
            nr.exchange_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
            return PT_OK;
        };
    }
    // a worker's failure: `device N[.j]: <message>`.  The fixed form reports the failure of the lowest device; in the adaptive form the first failure stops the
    // others (Lockstep) and is the one reported.
    std::vector<pt_status> status(n, PT_OK);
    std::vector<std::string> errors(n);
    std::vector<pt_profile> profiles(n);
    const auto t0 = std::chrono::steady_clock::now();
    node_run(n, [&](int v) {
        pt_status s2 = hipSetDevice(node.devices[v / virt]) == hipSuccess ? PT_OK : fail(PT_ERR_DEVICE, "hipSetDevice failed");
        pt_render_desc rv = rd;
        if (n > 1) { rv.shard_index = (uint32_t)v; rv.shard_count = (uint32_t)n; }
        pt_scene* s = node.scene_of[v];
        RenderJob job;
        if (adaptive) { job.adaptive = call.ad; job.node = &nr; job.node_index = v; }
        if (call.sd) { job.d_spectral = s->spectral_cache.as<float>(); job.spectral_bins = call.sd->bins; job.shard_list = &s->spectral_shard.px; }
        // (a shard together with groups: the one-device entries refuse it in check_light_groups_args, which this driver's callers do not run on a worker's desc)
        const LightGroupTable table{s->group_table.as<uint8_t>(), call.gd ? call.gd->environment_group : 0u, call.gd ? call.gd->group_count : 0u};
        if (call.gd) { job.groups = &table; job.d_group_films = s->group_films_cache.as<float>(); job.shard_list = &s->group_shard.px; }
        if (s2 == PT_OK) s2 = render_impl(s, &rv, m.films[v], m.streams[v], &profiles[v], job);
        if (s2 == PT_OK && call.sd) s2 = node_payload_exchange(m, node, ns, v);
        if (s2 == PT_OK && call.gd) s2 = node_payload_exchange(m, node, ng, v);
        if (s2 == PT_OK) return;
        status[v] = s2; errors[v] = device_name(node, v) + ": " + g_error;   // (g_error is thread-local: carried back to the caller below)
        if (adaptive) nr.lock.stop(s2, errors[v]);   // (a worker stopped by another's failure finds the first error kept)
    });
    if (nr.lock.failed) return fail(nr.lock.status, nr.lock.error);
    for (int v = 0; v < n; ++v) if (status[v] != PT_OK) return fail(status[v], errors[v]);
    // the only exchange step of the fixed path
    const auto t_gather = std::chrono::steady_clock::now();
    std::vector<GatherPart> parts = {GatherPart{std::vector<void*>(m.films.begin(), m.films.begin() + n), pixels * 4, ncclFloat}};
    if (adaptive) {
        parts.insert(parts.end(), {GatherPart{{}, pixels, ncclUint32}, GatherPart{{}, 2 * pixels, ncclFloat64}});
        for (int v = 0; v < n; ++v) { parts[1].bufs.push_back(node.scene_of[v]->adaptive.counts); parts[2].bufs.push_back(node.scene_of[v]->adaptive.stats); }
        if (!call.stats) parts.pop_back();
    }
    st = node_gather(m, node, parts);
    if (st != PT_OK) return st;
    const auto t_gathered = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(node.devices[0]));
    HIP_TRY(hipMemcpy(call.film, m.films[0], bytes, hipMemcpyDeviceToHost));
    if (adaptive) {
        HIP_TRY(hipMemcpy(call.sample_counts, node.scene_of[0]->adaptive.counts, sizeof(uint32_t) * pixels, hipMemcpyDeviceToHost));
        if (call.stats) HIP_TRY(hipMemcpy(call.stats, node.scene_of[0]->adaptive.stats, sizeof(double) * 2 * pixels, hipMemcpyDeviceToHost));
    }
    if (profile) {
        node_profile(profiles, profile);
        // seconds: the workers and the gather for the fixed form; for the adaptive form the whole call (set-up, rounds, gather, read-backs)
        profile->seconds = std::chrono::duration<double>(adaptive ? std::chrono::steady_clock::now() - t_entry : t_gathered - t0).count();
        if (adaptive) profile->kernel_launches[5] = profiles[0].kernel_launches[5];                        // the rounds (every device ran them all)
        profile->kernel_seconds[5] = std::chrono::duration<double>(t0 - t_entry).count();    // set-up (replicas, streams, films, communicator): ~0 on a repeated call
        // the rounds' exchanges (adaptive) + the film reduce or gather (+ the longest pack, copy and scatter)
        profile->kernel_seconds[6] = nr.exchange_seconds + std::chrono::duration<double>(t_gathered - t_gather).count() + node_payload_seconds(ns) + node_payload_seconds(ng);
    }
    // the node render has succeeded: the scene's resident film, or its resident group films (paired with no resident film), are the packed shards
    if (call.sd) {
        sc->spectral_shards = node.scene_of;
        sc->spectral_width = rd.width; sc->spectral_height = rd.height; sc->spectral_bins = call.sd->bins; sc->spectral_valid = true;
    }
    if (call.gd) {
        sc->group_shards = node.scene_of;
        sc->groups_width = rd.width; sc->groups_height = rd.height; sc->groups_count = call.gd->group_count; sc->groups_valid = true;
    }
    if (adaptive) {   // where the pieces lie, for pt_resident_assemble: no device work, and nothing is resident (include/pt_resident.h)
        NodeRemembered& k = m.node_render;
        k.info.valid = true; k.info.stats = call.stats != nullptr;
        k.info.width = rd.width; k.info.height = rd.height; k.info.bins = call.sd ? call.sd->bins : 0u;
        k.device = node.devices[0];
        k.film = m.films[0]; k.counts = node.scene_of[0]->adaptive.counts; k.stats = node.scene_of[0]->adaptive.stats;
        if (call.sd) k.spectral = {node.scene_of, call.sd->bins};
        if (call.gd) k.groups = {node.scene_of, call.gd->group_count};
    }
    return PT_OK;
}

pt_status pt_render_multi(pt_scene* sc, const pt_render_desc* rdp, uint64_t device_mask, float* film, pt_profile* profile) {
    forget_node_render(sc);
    if (!sc || !rdp || !film) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (rdp->width == 0 || rdp->height == 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (rdp->shard_count > 1) return fail(PT_ERR_INVALID_ARGUMENT, "pt_render_multi deals the tiles itself: shard_count must be 0");
    RenderCall call;
    call.rd = rdp; call.film = film;
    return render_node(sc, call, device_mask, profile);
}

pt_status pt_render_spectral_multi(pt_scene* sc, const pt_render_desc* rdp, const pt_spectral_desc* sdp, uint64_t device_mask, float* film, float* spectral,
                                   pt_profile* profile) {
    if (sc) { sc->spectral_valid = false; sc->spectral_shards.clear(); }   // (a spectral render starts; whatever it is refused for, no film is resident after it)
    forget_node_render(sc);
    pt_render_desc rd;
    std::string err;
    const pt_status st = pth::check_spectral_multi_args(sc, rdp, sdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, film, spectral, &rd, &err);
    if (st != PT_OK) return fail(st, err);
    RenderCall call;
    call.rd = &rd; call.sd = sdp; call.film = film; call.spectral = spectral;
    return render_node(sc, call, device_mask, profile);
}

pt_status pt_render_adaptive_multi(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, uint64_t device_mask, float* film,
                                   uint32_t* sample_counts, double* stats, pt_profile* profile) {
    forget_node_render(sc);
    if (!sc || !rdp || !adp || !film) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    const pt_status st = pth::normalize_adaptive_desc(*rdp, *adp, sample_counts != nullptr, (uint32_t)sc->host.cameras.size(), &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.film = film; call.sample_counts = sample_counts; call.stats = stats;
    return render_node(sc, call, device_mask, profile);
}

pt_status pt_render_adaptive_spectral_multi(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_spectral_desc* sdp, uint64_t device_mask,
                                            float* film, uint32_t* sample_counts, double* stats, float* spectral, pt_profile* profile) {
    if (sc) { sc->spectral_valid = false; sc->spectral_shards.clear(); }   // (as in pt_render_spectral_multi)
    forget_node_render(sc);
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    const pt_status st = pth::check_adaptive_spectral_args(sc, rdp, adp, sdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, film, sample_counts, spectral, &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.sd = sdp; call.film = film; call.sample_counts = sample_counts; call.stats = stats; call.spectral = spectral;
    return render_node(sc, call, device_mask, profile);
}

// include/pt_light_groups_multi.h.  A group call ends the residency of the group films before it, whatever it is refused for.
pt_status pt_render_light_groups_multi(pt_scene* sc, const pt_render_desc* rdp, const pt_light_groups_desc* gdp, uint64_t device_mask, float* film, float* group_films,
                                       pt_profile* profile) {
    end_group_films(sc);
    forget_node_render(sc);
    pt_render_desc rd;
    std::string err;
    const pt_status st = pth::check_light_groups_multi_args(sc, rdp, gdp, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, sc ? (uint32_t)sc->host.cameras.size() : 0u, film, &rd, &err);
    if (st != PT_OK) return fail(st, err);
    if ((uint64_t)rd.width * rd.height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = &rd; call.gd = gdp; call.film = film; call.group_films = group_films;
    return render_node(sc, call, device_mask, profile);
}

pt_status pt_render_adaptive_light_groups_multi(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, const pt_light_groups_desc* gdp, uint64_t device_mask,
                                                float* film, uint32_t* sample_counts, double* stats, float* group_films, pt_profile* profile) {
    end_group_films(sc);
    forget_node_render(sc);
    pt_render_desc rd;
    pt_adaptive_desc ad;
    std::string err;
    const pt_status st = pth::check_adaptive_light_groups_multi_args(sc, rdp, adp, gdp, sc ? sc->host.blob[PT_HDR_INSTANCE_COUNT] : 0u, sc ? (uint32_t)sc->host.cameras.size() : 0u,
                                                                     film, sample_counts, &rd, &ad, &err);
    if (st != PT_OK) return fail(st, err);
    if ((uint64_t)rd.width * rd.height > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive and width x height must fit 31 bits");
    RenderCall call;
    call.rd = &rd; call.ad = &ad; call.gd = gdp; call.film = film; call.sample_counts = sample_counts; call.stats = stats; call.group_films = group_films;
    return render_node(sc, call, device_mask, profile);
}

// ---- The probe pass: camera rays of chosen samples and their closest hits, behind pt_camera_samples, pt_intersect, the guide pass and the ID mattes.
// the RenderParams of a camera-ray probe of the render `rdp`: what stage_generate reads, nothing of the film
static RenderParams probe_params(const pt_scene* sc, const pt_render_desc* rdp) {
    RenderParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.seed = rdp->seed; rp.width = rdp->width; rp.height = rdp->height;
    rp.wavelength_lo = rdp->wavelength_lo; rp.wavelength_span = rdp->wavelength_hi - rdp->wavelength_lo;
    rp.camera = pth::camera_params(sc->host.cameras[rdp->camera_index], (float)rdp->width / (float)rdp->height);
    rp.chunk_pixels = 1;   // (stage_generate: sample = first_sample + slot / chunk_pixels — the probe hands the sample index in as the slot)
    return rp;
}
// the closest hits of the `n` rays (o, d) into `hits`: the probe kernel in the scene's own staging mode, on the null stream
static void launch_probe(const pt_scene* sc, uint32_t n, const float* o, const float* d, pt_hit* hits) {
    const int grid = sc->num_cus * 4;
    const uint32_t lds_bytes = sc->lds_mode == PT_LDS_ALL ? sc->blob_words * 4u : (sc->lds_mode == PT_LDS_CORE ? sc->host.blob[PT_HDR_CORE_WORDS] * 4u : 0u);
    launch_probe_intersect(LaunchCfg{grid, lds_bytes, (hipStream_t)0, sc->lds_mode}, SceneArgs{sc->d_blob, sc->blob_words, sc->d_tex}, n, o, d, hits);
}

pt_status pt_intersect(pt_scene* sc, size_t n, const float* origins, const float* directions, pt_hit* hits) {
    if (!sc || !origins || !directions || !hits) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(sc->device));
    DevBuf dor, dd, dh;
    HIP_TRY(dor.alloc(12 * n)); HIP_TRY(dd.alloc(12 * n)); HIP_TRY(dh.alloc(sizeof(pt_hit) * n));
    HIP_TRY(hipMemcpy(dor.p, origins, 12 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dd.p, directions, 12 * n, hipMemcpyHostToDevice));
    launch_probe(sc, (uint32_t)n, dor.as<float>(), dd.as<float>(), dh.as<pt_hit>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hits, dh.p, sizeof(pt_hit) * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_camera_samples(pt_scene* sc, const pt_render_desc* rdp, size_t n, const uint32_t* pixel, const uint32_t* sample, float* origins, float* directions, float* lambda) {
    if (!sc || !rdp || !pixel || !sample || !origins || !directions || !lambda) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (rdp->width == 0 || rdp->height == 0 || rdp->camera_index >= sc->host.cameras.size()) return fail(PT_ERR_INVALID_ARGUMENT, "width, height must be positive, camera_index in range");
    if (!(rdp->wavelength_hi >= rdp->wavelength_lo)) return fail(PT_ERR_INVALID_ARGUMENT, "wavelength_hi must not be below wavelength_lo");
    if (n > 0xffffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "at most 2^32 - 1 samples per call");
    const uint64_t n_pixels = (uint64_t)rdp->width * (uint64_t)rdp->height;   // (64-bit: a 32-bit product wraps for big films and lets ids through)
    if (n_pixels > 0xffffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "width x height must fit a 32-bit pixel id");
    for (size_t i = 0; i < n; ++i) if ((uint64_t)pixel[i] >= n_pixels) return fail(PT_ERR_INVALID_ARGUMENT, "pixel id out of range");
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(sc->device));
    const RenderParams rp = probe_params(sc, rdp);
    DevBuf dp, ds, dor, dd, dl;
    HIP_TRY(dp.alloc(4 * n)); HIP_TRY(ds.alloc(4 * n)); HIP_TRY(dor.alloc(12 * n)); HIP_TRY(dd.alloc(12 * n)); HIP_TRY(dl.alloc(4 * n));
    HIP_TRY(hipMemcpy(dp.p, pixel, 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ds.p, sample, 4 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_camera, dim3(256), dim3(kBlock), 0, 0, rp, (uint32_t)n, dp.as<uint32_t>(), ds.as<uint32_t>(), dor.as<float>(), dd.as<float>(), dl.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(origins, dor.p, 12 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(directions, dd.p, 12 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lambda, dl.p, 4 * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

// The albedo guide's tables for a render `rdp` of `sc`: the basis, material_row[m] (the first table row of material m's layers) and the curve values of every
// Lambertian material's texture layers at the basis wavelengths (one launch of k_albedo_tables).
// (rows_out, may be null: the number of table rows, for make_bin_albedo_table)
static pt_status make_albedo_tables(pt_scene* sc, const pt_render_desc* rdp, DnAlbedoBasis* basis, DevBuf* drow, DevBuf* dloff, DevBuf* dtable, uint32_t* rows_out = nullptr) {
    const uint32_t materials = sc->host.material_count;
    // the table's rows: the layers of every Lambertian material's texture stack, in material order (a stack two materials share gets two sets of rows)
    const std::vector<uint32_t>& blob = sc->host.blob;
    std::vector<uint32_t> material_row(materials ? materials : 1u, 0u), layer_off;
    for (uint32_t m = 0; m < materials; ++m) {
        const uint32_t rec = blob[PT_HDR_MATERIAL_OFF] + m * PT_MAT_WORDS;
        if (blob[rec + PT_MAT_KIND] != (uint32_t)PT_MATERIAL_LAMBERTIAN) continue;
        const uint32_t ts = blob[rec + PT_MAT_TEXSTACK];
        material_row[m] = (uint32_t)layer_off.size();
        for (uint32_t i = 0; i < blob[ts]; ++i) layer_off.push_back(ts + 1u + i * PT_LAYER_WORDS);
    }
    const uint32_t rows = (uint32_t)layer_off.size();
    albedo_basis(rdp->wavelength_lo, rdp->wavelength_hi, basis);
    HIP_TRY(drow->alloc(4 * material_row.size())); HIP_TRY(dloff->alloc(4 * (size_t)(rows ? rows : 1u))); HIP_TRY(dtable->alloc(16 * (size_t)(rows ? rows : 1u) * DN_ALBEDO_WAVELENGTHS));
    HIP_TRY(hipMemcpy(drow->p, material_row.data(), 4 * material_row.size(), hipMemcpyHostToDevice));
    if (rows) HIP_TRY(hipMemcpy(dloff->p, layer_off.data(), 4 * (size_t)rows, hipMemcpyHostToDevice));
    launch_albedo_tables(sc->d_blob, sc->d_tex, *basis, rows, dloff->as<uint32_t>(), dtable->as<float>());
    if (rows_out) *rows_out = rows;
    return PT_OK;
}
// The per-bin albedo guide's table and sums (include/pt_spectral.h pt_render_guides_bin_albedo): the curve values of make_albedo_tables' rows at the centres of
// the render's `bins` wavelength bins (one launch of k_bin_albedo_tables), and bins x n zeroed running sums.  *fold: what the fold kernels take.
// (sums: device planes of the caller's that the sums, and at the end the per-bin albedo, are to lie in; null = dbsum, allocated here)
static pt_status make_bin_albedo_fold(pt_scene* sc, const pt_render_desc* rdp, uint32_t bins, uint32_t n, uint32_t rows, const DevBuf& drow, const DevBuf& dloff, DevBuf* dbtable,
                                      DevBuf* dbsum, float* sums, BinAlbedoFold* fold) {
    HIP_TRY(dbtable->alloc(16 * (size_t)(rows ? rows : 1u) * bins));
    if (!sums) { HIP_TRY(dbsum->alloc(4 * (size_t)bins * n)); sums = dbsum->as<float>(); }
    HIP_TRY(hipMemsetAsync(sums, 0, 4 * (size_t)bins * n, 0));
    launch_bin_albedo_tables(sc->d_blob, sc->d_tex, rdp->wavelength_lo, dn_bin_width(rdp->wavelength_lo, rdp->wavelength_hi, bins), bins, rows, dloff.as<uint32_t>(),
                             dbtable->as<float>());
    *fold = BinAlbedoFold{sums, reinterpret_cast<const float4*>(dbtable->p), drow.as<uint32_t>(), bins, n};
    return PT_OK;
}
// include/pt_denoise.h: the guides of the film denoiser.  Per sample index k the camera rays of every pixel (stage_generate, as pt_camera_samples runs it), the
// closest hits as pt_intersect finds them (the probe kernel in the scene's own staging mode), and the fold of the hit records in k order (pt_denoise.hip).
// `albedo` (may be null): include/pt_denoise.h's second guide, from the same hit records — the fold and the division then run in their albedo forms, after one
// launch that tabulates the curves of the Lambertian materials' texture layers at the basis wavelengths.  `bin_albedo` (may be null; needs albedo): the per-bin
// albedo over `bins` bins from the same hit records, folded by a second kernel behind the fold.
// Where the outputs of a guide pass go: host arrays, copied out of device buffers of the call's own — or (device) buffers on the scene's device that the
// last kernels write where they lie (pt_resident_guides).  That is the only difference between the two.
struct GuideOut {
    float* guides; float* albedo; float* bin_albedo; bool device;
};
// `chain` (null: the first hit, as above): the guides at the end of every sample's specular chain.  Per sample index the camera rays go out as a list with the
// identity pixel order; per chain vertex the probe runs over the rays still on their way and k_chain_step (pt_guides_chain.hip) folds the ones that end into
// their pixels' sums and compacts the rest into the next list, whose length comes back in one 4-byte read — the probe's launcher takes its ray count by value.
// The last possible vertex (v == max_chain) ends every ray, so nothing is read back after it.  The per-bin albedo is folded by k_chain_step at the same
// terminal vertex.  The two forms share their buffers, tables and finish and differ in their loops — and in who zeroes the sums: the first-hit folds do at
// k == 0, the chain form clears them up front, since a pixel's first sample may end at any vertex.
static pt_status render_guides_impl(pt_scene* sc, const pt_render_desc* rdp, uint32_t guide_samples, const pt_guide_chain_desc* chain, const GuideOut& out, uint32_t bins = 0) {
    float *const guides = out.guides, *const albedo = out.albedo, *const bin_albedo = out.bin_albedo;
    HIP_TRY(hipSetDevice(sc->device));
    const uint32_t n = rdp->width * rdp->height, materials = sc->host.material_count;
    const RenderParams rp = probe_params(sc, rdp);
    DevBuf dor[2], dd[2], dstate[2], dh, dsum, dg, dasum, da, drow, dloff, dtable, dcount, dbtable, dbsum;   // (the second ray list, dstate and dcount: the chain's)
    for (int i = 0; i < (chain ? 2 : 1); ++i) {
        HIP_TRY(dor[i].alloc(12 * (size_t)n)); HIP_TRY(dd[i].alloc(12 * (size_t)n));
        if (chain) HIP_TRY(dstate[i].alloc(16 * (size_t)n));
    }
    HIP_TRY(dh.alloc(sizeof(pt_hit) * (size_t)n)); HIP_TRY(dsum.alloc(sizeof(DnGuideSum) * (size_t)n));
    float *d_guides = guides, *d_albedo = albedo;
    if (!out.device) { HIP_TRY(dg.alloc(16 * (size_t)n)); d_guides = dg.as<float>(); }
    if (chain) {
        HIP_TRY(dcount.alloc(4 * (size_t)(chain->max_chain + 1u)));
        HIP_TRY(hipMemsetAsync(dsum.p, 0, sizeof(DnGuideSum) * (size_t)n, 0));
    }
    ChainAlbedo ca;   // (the albedo sums, tables and per-bin fold of either form)
    memset(&ca, 0, sizeof(ca));
    if (albedo) {
        HIP_TRY(dasum.alloc(16 * (size_t)n));
        if (!out.device) { HIP_TRY(da.alloc(16 * (size_t)n)); d_albedo = da.as<float>(); }
        if (chain) HIP_TRY(hipMemsetAsync(dasum.p, 0, 16 * (size_t)n, 0));
        uint32_t rows = 0;
        const pt_status ast = make_albedo_tables(sc, rdp, &ca.basis, &drow, &dloff, &dtable, &rows);
        if (ast != PT_OK) return ast;
        ca.albedo_sums = dasum.as<float>(); ca.material_row = drow.as<uint32_t>(); ca.table = dtable.as<float>();
        if (bin_albedo) {
            const pt_status bst = make_bin_albedo_fold(sc, rdp, bins, n, rows, drow, dloff, &dbtable, &dbsum, out.device ? bin_albedo : nullptr, &ca.bin_fold);
            if (bst != PT_OK) return bst;
        }
    }
    const ChainRays rays[2] = {{dor[0].as<float>(), dd[0].as<float>(), dstate[0].as<uint4>()}, {dor[1].as<float>(), dd[1].as<float>(), dstate[1].as<uint4>()}};
    if (!chain) for (uint32_t k = 0; k < guide_samples; ++k) {
        launch_guide_rays(rp, n, k, rays[0].o, rays[0].d);
        launch_probe(sc, n, rays[0].o, rays[0].d, dh.as<pt_hit>());
        if (albedo)
            launch_guide_fold_albedo(n, dh.as<pt_hit>(), dsum.as<DnGuideSum>(), ca.albedo_sums, k == 0, sc->d_blob, sc->d_tex, materials, ca.material_row, ca.table, ca.basis);
        else
            launch_guide_fold(n, dh.as<pt_hit>(), dsum.as<DnGuideSum>(), k == 0);
        if (ca.bin_fold.sums) launch_guide_fold_bins(n, dh.as<pt_hit>(), ca.bin_fold, sc->d_blob, sc->d_tex, materials);
    }
    else for (uint32_t k = 0; k < guide_samples; ++k) {
        launch_chain_rays(rp, n, k, rays[0]);
        HIP_TRY(hipMemsetAsync(dcount.p, 0, 4 * (size_t)(chain->max_chain + 1u), 0));
        uint32_t active = n;
        for (uint32_t v = 0; v <= chain->max_chain && active != 0u; ++v) {
            const ChainRays &in = rays[v & 1u], &next = rays[(v & 1u) ^ 1u];
            launch_probe(sc, active, in.o, in.d, dh.as<pt_hit>());
            launch_chain_step(active, dh.as<pt_hit>(), in, next, dcount.as<uint32_t>() + v, dsum.as<DnGuideSum>(), ca, v, chain->max_chain, chain->alpha_max, sc->d_blob, sc->d_tex,
                              materials);
            if (v == chain->max_chain) break;
            HIP_TRY(hipMemcpy(&active, dcount.as<uint32_t>() + v, 4, hipMemcpyDeviceToHost));
            if (active > n) return fail(PT_ERR_DEVICE, "the chain's ray list grew");   // (never: a launch appends at most its own rays)
        }
    }
    if (albedo) launch_guide_finish_albedo(n, dsum.as<DnGuideSum>(), dasum.as<float>(), guide_samples, d_guides, d_albedo);
    else launch_guide_finish(n, dsum.as<DnGuideSum>(), guide_samples, d_guides);
    if (ca.bin_fold.sums) launch_bin_albedo_finish(n, bins, ca.bin_fold.sums, guide_samples, ca.bin_fold.sums);   // (in place: one value per lane)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (out.device) return PT_OK;
    HIP_TRY(hipMemcpy(guides, d_guides, 16 * (size_t)n, hipMemcpyDeviceToHost));
    if (albedo) HIP_TRY(hipMemcpy(albedo, d_albedo, 16 * (size_t)n, hipMemcpyDeviceToHost));
    if (ca.bin_fold.sums) HIP_TRY(hipMemcpy(bin_albedo, ca.bin_fold.sums, 4 * (size_t)bins * n, hipMemcpyDeviceToHost));
    return PT_OK;
}
pt_status pt_render_guides(pt_scene* sc, const pt_render_desc* rdp, uint32_t guide_samples, float* guides) {
    std::string err;
    const pt_status st = pth::check_guides_args(sc, rdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, guides, &err);
    if (st != PT_OK) return fail(st, err);
    return render_guides_impl(sc, rdp, guide_samples, nullptr, GuideOut{guides, nullptr, nullptr, false});
}
pt_status pt_render_guides_albedo(pt_scene* sc, const pt_render_desc* rdp, uint32_t guide_samples, float* guides, float* albedo) {
    std::string err;
    const pt_status st = pth::check_guides_args(sc, rdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, guides, &err);
    if (st != PT_OK) return fail(st, err);
    if (!albedo) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    return render_guides_impl(sc, rdp, guide_samples, nullptr, GuideOut{guides, albedo, nullptr, false});
}

// include/pt_denoise.h: the ID mattes.  Per sample index the launches of a guide pass — the camera rays of every pixel, their closest hits — and behind them
// k_matte_fold (pt_matte.hip), which folds the hit records' instance or material into the pixels' slots; the launch of sample 0 initialises the table.  The finish
// sorts and divides into the scene's resident planes, which the outputs asked for are copied from.
pt_status pt_render_mattes(pt_scene* sc, const pt_render_desc* rdp, const pt_matte_desc* mdp, uint32_t* keys, float* coverage, uint32_t* overflow) {
    std::string err;
    const pt_status st = pth::check_matte_args(sc, rdp, mdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, &err);
    if (st != PT_OK) return fail(st, err);
    HIP_TRY(hipSetDevice(sc->device));
    sc->mattes_valid = false;
    const uint32_t n = rdp->width * rdp->height, ranks = mdp->ranks, samples = mdp->samples;
    const RenderParams rp = probe_params(sc, rdp);
    const size_t plane_bytes = 4 * (size_t)ranks * n;
    pt_status cached = sc->matte_keys.reserve(plane_bytes);
    if (cached == PT_OK) cached = sc->matte_coverage.reserve(plane_bytes);
    if (cached != PT_OK) return cached;
    DevBuf dor, dd, dh, dtable, doverflow;
    HIP_TRY(dor.alloc(12 * (size_t)n)); HIP_TRY(dd.alloc(12 * (size_t)n)); HIP_TRY(dh.alloc(sizeof(pt_hit) * (size_t)n));
    HIP_TRY(dtable.alloc(ptk::matte_table_bytes(n, ranks))); HIP_TRY(doverflow.alloc(4 * (size_t)n));
    for (uint32_t k = 0; k < samples; ++k) {
        launch_guide_rays(rp, n, k, dor.as<float>(), dd.as<float>());
        launch_probe(sc, n, dor.as<float>(), dd.as<float>(), dh.as<pt_hit>());
        HIP_TRY(ptk::launch_matte_fold(nullptr, n, ranks, mdp->key, dh.as<pt_hit>(), dtable.p, k == 0));
    }
    HIP_TRY(ptk::launch_matte_finish(nullptr, n, ranks, samples, dtable.p, sc->matte_keys.as<uint32_t>(), sc->matte_coverage.as<float>(), doverflow.as<uint32_t>()));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (keys) HIP_TRY(hipMemcpy(keys, sc->matte_keys.p, plane_bytes, hipMemcpyDeviceToHost));
    if (coverage) HIP_TRY(hipMemcpy(coverage, sc->matte_coverage.p, plane_bytes, hipMemcpyDeviceToHost));
    if (overflow) HIP_TRY(hipMemcpy(overflow, doverflow.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    sc->mattes_valid = true;
    sc->matte_width = rdp->width; sc->matte_height = rdp->height; sc->matte_ranks = ranks; sc->matte_samples = samples;
    return PT_OK;
}

pt_status pt_mattes_resident(pt_scene* sc, uint32_t* width, uint32_t* height, uint32_t* ranks, uint32_t* samples) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!width || !height || !ranks || !samples) return fail(PT_ERR_INVALID_ARGUMENT, "width, height, ranks or samples is null");
    if (!sc->mattes_valid) return fail(PT_ERR_INVALID_ARGUMENT, "the scene has no resident matte: pt_render_mattes must have succeeded on it");
    *width = sc->matte_width; *height = sc->matte_height; *ranks = sc->matte_ranks; *samples = sc->matte_samples;
    return PT_OK;
}

// pt_matte_extract's kernel over the resident planes, on the stream the render ran on (the null stream): the selections go up, set_count planes come back
pt_status pt_matte_extract_resident(pt_scene* sc, uint32_t set_count, const uint32_t* offsets, const uint32_t* selected, float* out) {
    if (!sc) return fail(PT_ERR_INVALID_ARGUMENT, "the scene is null");
    if (!sc->mattes_valid) return fail(PT_ERR_INVALID_ARGUMENT, "the scene has no resident matte: pt_render_mattes must have succeeded on it");
    std::string err;
    const pt_status st = pth::check_matte_selections(set_count, offsets, selected, out, &err);
    if (st != PT_OK) return fail(st, err);
    if (set_count == 0) return PT_OK;
    std::vector<uint32_t> selection;
    pth::matte_selection_words(set_count, offsets, selected, &selection);
    HIP_TRY(hipSetDevice(sc->device));
    const size_t n_pixels = (size_t)sc->matte_width * sc->matte_height;
    return apply_resident(sc, &pt_scene::matte_extract_cache, ptk::kMatteSelectionWords, selection.data(), 4 * selection.size(), out, 4 * (size_t)set_count * n_pixels,
                          [&](float* d_words, float* d_out, hipStream_t stream) {
                              const uint32_t* d_selection = reinterpret_cast<const uint32_t*>(d_words);   // (32-bit words in the float-typed cache)
                              return ptk::launch_matte_extract(ptk::matte_extract_grid(sc->num_cus, (uint32_t)n_pixels), stream, (uint32_t)n_pixels, sc->matte_ranks,
                                                               sc->matte_keys.as<uint32_t>(), sc->matte_coverage.as<float>(), set_count, d_selection,
                                                               d_selection + ptd::MATTE_SETS_MAX + 1u, d_out);
                          });
}

pt_status pt_render_guides_chain(pt_scene* sc, const pt_render_desc* rdp, uint32_t guide_samples, const pt_guide_chain_desc* chain, float* guides, float* albedo) {
    std::string err;
    pt_guide_chain_desc cd;
    const pt_status st = pth::check_guides_chain_args(sc, rdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, chain, guides, &cd, &err);
    if (st != PT_OK) return fail(st, err);
    return render_guides_impl(sc, rdp, guide_samples, &cd, GuideOut{guides, albedo, nullptr, false});
}
// include/pt_spectral.h: the guides, the XYZ albedo and the per-bin albedo from one set of probes — at the first hit, or with a chain of max_chain > 0 at the
// end of every sample's specular chain (render_guides_impl's two loops).  The XYZ albedo is always computed (its tables' rows are the per-bin
// table's); a caller that passes none gets none.
pt_status pt_render_guides_bin_albedo(pt_scene* sc, const pt_render_desc* rdp, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t bins, float* guides,
                                      float* albedo, float* bin_albedo) {
    std::string err;
    pt_guide_chain_desc cd;
    const pt_status st = pth::check_guides_bin_albedo_args(sc, rdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, chain, bins, guides, bin_albedo, &cd, &err);
    if (st != PT_OK) return fail(st, err);
    std::vector<float> own_albedo;
    if (!albedo) { own_albedo.resize(4 * (size_t)rdp->width * rdp->height); albedo = own_albedo.data(); }
    return render_guides_impl(sc, rdp, guide_samples, cd.max_chain ? &cd : nullptr, GuideOut{guides, albedo, bin_albedo, false}, bins);
}

// ---- include/pt_resident.h.  Every argument, and what the call needs resident, is checked by pth::check_resident_* before a device is looked for.
static struct pt_resident_info resident_now(const pt_scene* sc) {
    if (sc) return sc->resident.info();
    struct pt_resident_info none;
    memset(&none, 0, sizeof(none));
    return none;
}
pt_status pt_resident_info(pt_scene* sc, struct pt_resident_info* info) {
    std::string err;
    const pt_status st = pth::check_resident_info_args(sc, info, &err);
    if (st != PT_OK) return fail(st, err);
    *info = sc->resident.info();
    return PT_OK;
}
// the guide pass of the host-array entries with its outputs kept: the same launches on the same stream, the last of them writing the scene's buffers
pt_status pt_resident_guides(pt_scene* sc, const pt_render_desc* rdp, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t flags) {
    std::string err;
    pt_guide_chain_desc cd;
    pt_status st = pth::check_resident_guides_args(sc, rdp, sc ? (uint32_t)sc->host.cameras.size() : 0u, guide_samples, chain, flags, resident_now(sc), &cd, &err);
    if (st != PT_OK) return fail(st, err);
    ResidentSet& r = sc->resident;
    HIP_TRY(hipSetDevice(sc->device));
    const size_t np = (size_t)r.width * r.height;
    r.parts &= ~(PT_RESIDENT_GUIDES | PT_RESIDENT_ALBEDO | PT_RESIDENT_BIN_ALBEDO | PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    r.tidy();
    const bool albedo = (flags & PT_RESIDENT_ALBEDO) != 0u, bin_albedo = (flags & PT_RESIDENT_BIN_ALBEDO) != 0u;
    st = r.guides.reserve(16 * np);
    if (st == PT_OK && albedo) st = r.albedo.reserve(16 * np);
    if (st == PT_OK && bin_albedo) st = r.bin_albedo.reserve(4 * np * r.bins);
    if (st != PT_OK) return st;
    const GuideOut out{r.guides.as<float>(), albedo ? r.albedo.as<float>() : nullptr, bin_albedo ? r.bin_albedo.as<float>() : nullptr, true};
    st = render_guides_impl(sc, rdp, guide_samples, cd.max_chain ? &cd : nullptr, out, bin_albedo ? r.bins : 0u);
    if (st != PT_OK) return st;
    r.parts |= PT_RESIDENT_GUIDES | (albedo ? PT_RESIDENT_ALBEDO : 0u) | (bin_albedo ? PT_RESIDENT_BIN_ALBEDO : 0u);
    return PT_OK;
}
pt_status pt_resident_load(pt_scene* sc, uint32_t width, uint32_t height, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats,
                           const float* spectral, const float* guides, const float* albedo, const float* bin_albedo) {
    std::string err;
    pt_status st = pth::check_resident_load_args(sc, width, height, bins, film, sample_counts, stats, spectral, guides, albedo, bin_albedo, resident_now(sc), &err);
    if (st != PT_OK) return fail(st, err);
    ResidentSet& r = sc->resident;
    HIP_TRY(hipSetDevice(sc->device));
    const size_t np = (size_t)width * height;
    // a part that is given is resident no longer until its upload has succeeded; the denoised parts go with the inputs they came from
    if (film) sc->groups_paired = false;   // (the film the group films came with is replaced)
    r.parts &= ~((film ? PT_RESIDENT_FILM : 0u) | (spectral ? PT_RESIDENT_BINS : 0u) | (guides ? PT_RESIDENT_GUIDES : 0u) | (albedo ? PT_RESIDENT_ALBEDO : 0u) |
                 (bin_albedo ? PT_RESIDENT_BIN_ALBEDO : 0u) | PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    r.tidy();
    struct Part { GrowBuf* buf; const void* host; size_t bytes; };
    const Part parts[] = {{&r.load_film, film, 16 * np}, {&r.load_counts, sample_counts, 4 * np}, {&r.load_stats, stats, 16 * np}, {&r.load_spectral, spectral, 4 * np * bins},
                          {&r.guides, guides, 16 * np}, {&r.albedo, albedo, 16 * np}, {&r.bin_albedo, bin_albedo, 4 * np * bins}};
    for (const Part& p : parts) {
        if (!p.host) continue;
        st = p.buf->reserve(p.bytes);
        if (st != PT_OK) return st;
        HIP_TRY(hipMemcpy(p.buf->p, p.host, p.bytes, hipMemcpyHostToDevice));
    }
    if (film) { r.film = r.load_film.as<float>(); r.counts = r.load_counts.as<uint32_t>(); r.stats = r.load_stats.as<double>(); r.parts |= PT_RESIDENT_FILM; }
    if (spectral) { r.spectral = r.load_spectral.as<float>(); r.parts |= PT_RESIDENT_BINS; }
    if (guides) r.parts |= PT_RESIDENT_GUIDES;
    if (albedo) r.parts |= PT_RESIDENT_ALBEDO;
    if (bin_albedo) r.parts |= PT_RESIDENT_BIN_ALBEDO;
    r.width = width; r.height = height;
    if (spectral || bin_albedo) r.bins = bins;
    return PT_OK;
}
// The pieces of the last adaptive node render gathered on the scene's device, device to device, on the null stream (the stream of the guide pass and the filter).
// The shards are disjoint and cover the film, so the planes are not zeroed and every float of them is written exactly once.
pt_status pt_resident_assemble(pt_scene* sc, uint32_t flags) {
    std::string err;
    pt_status st = pth::check_resident_assemble(sc, flags, sc ? sc->multi.node_render.info : pth::NodeRender(), &err);
    if (st != PT_OK) return fail(st, err);
    const NodeRemembered& k = sc->multi.node_render;
    ResidentSet& r = sc->resident;
    DeviceGuard guard;
    HIP_TRY(hipSetDevice(sc->device));
    r.end();   // (every part is replaced or belonged to another film; on any failure below nothing is resident)
    sc->groups_paired = false;
    const size_t np = (size_t)k.info.width * k.info.height;
    const uint32_t bins = k.info.bins;
    const bool staged_all = (flags & PT_RESIDENT_ASSEMBLE_STAGED) != 0u;
    // a shard is staged when it lies on another device (or every one, on request); its pixel list is uploaded unless a replica on this device still holds it
    const auto staged = [&](const pt_scene* s) { return staged_all || s->device != sc->device; };
    const auto listed = [&](const pt_scene* s) { return s != sc && s->device == sc->device; };
    // what the shards of a kind need: floats of staging and words of uploaded lists
    const auto need = [&](const NodeRemembered::Shards& set, const ShardKind& kind, size_t* staging_floats, size_t* px_words) {
        for (const pt_scene* s : set.scenes) {
            const size_t n_own = (s->*kind.shard).px.size();
            if (staged(s)) *staging_floats += (size_t)kind.floats * set.planes * n_own;
            if (!listed(s)) *px_words += n_own;
        }
    };
    // (a group render's shards are staged behind the bins' on a 16-byte boundary: pixels of four floats)
    size_t bin_floats = 0, group_floats = 0, px_words = 0;
    need(k.spectral, kSpectralShard, &bin_floats, &px_words);
    need(k.groups, kGroupShard, &group_floats, &px_words);
    const uint32_t groups = k.groups.planes;
    const size_t group_stage_first = (bin_floats + 3) & ~(size_t)3, staging_floats = group_floats ? group_stage_first + group_floats : bin_floats;
    if (!k.groups.scenes.empty()) end_group_films(sc);   // (the shards are unpacked below: on any failure no group films are resident)
    st = r.load_film.reserve(16 * np);
    if (st == PT_OK) st = r.load_counts.reserve(4 * np);
    if (st == PT_OK) st = r.load_stats.reserve(16 * np);
    if (st == PT_OK && bins) st = r.load_spectral.reserve(4 * np * bins);
    if (st == PT_OK && !k.groups.scenes.empty()) st = sc->group_films_cache.reserve(16 * np * groups);
    if (st == PT_OK && staging_floats) st = sc->assemble_staging.reserve(sizeof(float) * staging_floats);
    if (st == PT_OK && px_words) st = sc->assemble_px.reserve(sizeof(uint32_t) * px_words);
    if (st != PT_OK) return st;
    const hipStream_t stream = nullptr;
    const bool film_peer = k.device != sc->device;
    const auto film_copy = [&](void* dst, const void* src, size_t bytes) {
        return film_peer ? hipMemcpyPeerAsync(dst, sc->device, src, k.device, bytes, stream) : hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream);
    };
    HIP_TRY(film_copy(r.load_film.p, k.film, 16 * np));
    HIP_TRY(film_copy(r.load_counts.p, k.counts, 4 * np));
    HIP_TRY(film_copy(r.load_stats.p, k.stats, 16 * np));
    uint32_t* lists = sc->assemble_px.as<uint32_t>();
    // the shards of a kind unpacked into `full`, staged from `stage` on
    const auto unpack = [&](const NodeRemembered::Shards& set, const ShardKind& kind, float* stage, float* full) -> pt_status {
        for (const pt_scene* s : set.scenes) {
            const Shard& shard = s->*kind.shard;
            const uint32_t n_own = (uint32_t)shard.px.size();
            if (n_own == 0) continue;   // (a shard without a pixel moves nothing and launches nothing)
            const size_t floats = (size_t)kind.floats * set.planes * n_own;
            const float* packed = shard.packed.as<float>();
            if (staged(s)) {
                HIP_TRY(hipMemcpyPeerAsync(stage, sc->device, packed, s->device, sizeof(float) * floats, stream));   // (legal within one device too)
                packed = stage;
                stage += floats;
            }
            const uint32_t* px = s->buf.pixels;   // (the list its render left there)
            if (!listed(s)) {
                HIP_TRY(hipMemcpyAsync(lists, shard.px.data(), sizeof(uint32_t) * n_own, hipMemcpyHostToDevice, stream));
                px = lists;
                lists += n_own;
            }
            HIP_TRY(ptk::launch_shard_unpack(kind.floats, ptk::shard_pack_grid(sc->num_cus, n_own), stream, packed, px, n_own, set.planes, full, (uint32_t)np));
        }
        return PT_OK;
    };
    st = unpack(k.spectral, kSpectralShard, sc->assemble_staging.as<float>(), r.load_spectral.as<float>());
    // the group films of an adaptive node group render, into the buffer a one-device group render leaves them in
    if (st == PT_OK) st = unpack(k.groups, kGroupShard, sc->assemble_staging.as<float>() + group_stage_first, sc->group_films_cache.as<float>());
    if (st != PT_OK) return st;
    HIP_TRY(hipStreamSynchronize(stream));
    r.parts = PT_RESIDENT_FILM | (bins ? PT_RESIDENT_BINS : 0u);
    r.width = k.info.width; r.height = k.info.height; r.bins = bins;
    r.film = r.load_film.as<float>(); r.counts = r.load_counts.as<uint32_t>(); r.stats = r.load_stats.as<double>();
    r.spectral = bins ? r.load_spectral.as<float>() : nullptr;
    if (!k.groups.scenes.empty()) {   // (the group films lie beside the film they were rendered with, as after pt_render_adaptive_light_groups)
        sc->groups_width = k.info.width; sc->groups_height = k.info.height; sc->groups_count = groups;
        sc->groups_valid = true; sc->groups_paired = true;
    }
    return PT_OK;
}
pt_status pt_resident_read(pt_scene* sc, float* film, uint32_t* sample_counts, double* stats, float* spectral) {
    std::string err;
    const pt_status st = pth::check_resident_read_args(sc, film, sample_counts, stats, spectral, resident_now(sc), &err);
    if (st != PT_OK) return fail(st, err);
    const ResidentSet& r = sc->resident;
    DeviceGuard guard;
    HIP_TRY(hipSetDevice(sc->device));
    const size_t np = (size_t)r.width * r.height;
    const hipStream_t stream = nullptr;
    if (film) HIP_TRY(hipMemcpyAsync(film, r.film, 16 * np, hipMemcpyDeviceToHost, stream));
    if (sample_counts) HIP_TRY(hipMemcpyAsync(sample_counts, r.counts, 4 * np, hipMemcpyDeviceToHost, stream));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, r.stats, 16 * np, hipMemcpyDeviceToHost, stream));
    if (spectral) HIP_TRY(hipMemcpyAsync(spectral, r.spectral, 4 * np * r.bins, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}
// ---- What the two resident filters share.  The scratch of the film's passes on the resident set (it holds nothing between calls), then the entry's `own`
// buffers, in that order; a want of zero bytes is skipped.
struct Want { GrowBuf* buf; size_t bytes; };
static pt_status reserve_filter_buffers(ResidentSet& r, size_t np, std::initializer_list<Want> own) {
    std::vector<Want> wants = {{&r.color[0], 16 * np}, {&r.color[1], 16 * np}, {&r.geo, 16 * np}, {&r.tent, 4 * np}, {&r.flags, np}, {&r.grad, 8 * np}};
    wants.insert(wants.end(), own);
    for (const Want& w : wants) {
        const pt_status st = w.bytes ? w.buf->reserve(w.bytes) : PT_OK;
        if (st != PT_OK) return st;
    }
    return PT_OK;
}
// a run over the resident sources, albedo included where it is resident, with that scratch; everything else zero
static ptk::DnRun resident_filter_run(const ResidentSet& r) {
    ptk::DnRun run;
    memset(&run, 0, sizeof(run));
    run.film = r.film; run.counts = r.counts; run.stats = r.stats; run.guides = r.guides.as<float>();
    run.albedo = (r.parts & PT_RESIDENT_ALBEDO) ? r.albedo.as<float>() : nullptr;
    run.color[0] = r.color[0].as<float>(); run.color[1] = r.color[1].as<float>(); run.geo = r.geo.as<float>(); run.tent = r.tent.as<float>();
    run.flags = r.flags.as<uint8_t>(); run.grad = r.grad.as<float>();
    return run;
}
// the run's launches on the null stream, the outputs that are asked for back, and the synchronise.  `out_planes` (may be null): planes_bytes of what the run
// filtered beside the film — a group run's denoised group films, otherwise the denoised bins, which lie where dn_run says
static pt_status run_resident_filter(const pt_denoise_desc& d, ptk::DnRun* run, size_t np, float* out_film, float* out_variance, float* out_planes, size_t planes_bytes) {
    const hipStream_t stream = nullptr;
    ptk::dn_run(d, run, stream);
    HIP_TRY(hipGetLastError());
    if (out_film) HIP_TRY(hipMemcpyAsync(out_film, run->out_film, 16 * np, hipMemcpyDeviceToHost, stream));
    if (out_variance) HIP_TRY(hipMemcpyAsync(out_variance, run->out_variance, 4 * np, hipMemcpyDeviceToHost, stream));
    if (out_planes) HIP_TRY(hipMemcpyAsync(out_planes, run->groups ? run->out_groups : run->denoised_bins, planes_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}
// The filter where the film is: ptk::dn_run (pt_denoise.hip), the run the host-array entries make between their upload and their read-back, on the resident
// buffers and the null stream — the stream of the render and the guide pass.  The sources are read only; the scratch and the outputs are the scene's.
pt_status pt_denoise_resident(pt_scene* sc, const pt_resident_denoise_desc* desc, float* out_film, float* out_variance, float* out_spectral) {
    std::string err;
    pt_denoise_desc d;
    pt_status st = pth::check_resident_denoise_args(sc, desc, out_spectral, resident_now(sc), &d, &err);
    if (st != PT_OK) return fail(st, err);
    ResidentSet& r = sc->resident;
    HIP_TRY(hipSetDevice(sc->device));
    const size_t np = (size_t)r.width * r.height;
    const bool has_bins = (r.parts & PT_RESIDENT_BINS) != 0u, quads = has_bins && !(desc->flags & PT_RESIDENT_PLANAR_GATHER);
    r.parts &= ~(PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    const size_t bin_buf_bytes = has_bins ? ptk::dn_bin_buf_bytes(np, r.bins, quads) : 0;   // (without bins, and for den_bins without quads: zero bytes, skipped)
    st = reserve_filter_buffers(r, np, {{&r.den_film, 16 * np}, {&r.den_var, 4 * np}, {&r.bin_buf[0], bin_buf_bytes}, {&r.bin_buf[1], bin_buf_bytes},
                                        {&r.den_bins, quads ? 4 * np * r.bins : 0}});
    if (st != PT_OK) return st;
    ptk::DnRun run = resident_filter_run(r);
    if (has_bins) {
        run.bins = r.bins; run.spectral = r.spectral;
        run.bin_albedo = (r.parts & PT_RESIDENT_BIN_ALBEDO) ? r.bin_albedo.as<float>() : nullptr;
        run.bin_buf[0] = r.bin_buf[0].as<float>(); run.bin_buf[1] = r.bin_buf[1].as<float>();
        run.quads = quads; run.out_bins = quads ? r.den_bins.as<float>() : nullptr;
    }
    run.out_film = r.den_film.as<float>(); run.out_variance = r.den_var.as<float>();
    st = run_resident_filter(d, &run, np, out_film, out_variance, out_spectral, 4 * np * r.bins);
    if (st != PT_OK) return st;
    r.denoised_bins = run.denoised_bins;
    r.parts |= PT_RESIDENT_DENOISED | (has_bins ? PT_RESIDENT_DENOISED_BINS : 0u);
    return PT_OK;
}
// include/pt_light_groups_denoise.h: ptk::dn_run's group form on the resident film, guides and albedo and the group films paired with that film.  The scratch of the
// film's passes is pt_denoise_resident's (it holds nothing between calls); the outputs are this entry's own, so DENOISED and the buffers behind it stay as they are.
pt_status pt_denoise_light_groups_resident(pt_scene* sc, const pt_resident_denoise_desc* desc, float* out_film, float* out_variance, float* out_group_films) {
    std::string err;
    pt_denoise_desc d;
    pth::GroupsResident gr;
    if (sc) { gr.valid = sc->groups_valid; gr.paired = sc->groups_paired; gr.width = sc->groups_width; gr.height = sc->groups_height; gr.group_count = sc->groups_count; }
    pt_status st = pth::check_resident_denoise_light_groups_args(sc, desc, resident_now(sc), gr, &d, &err);
    if (st != PT_OK) return fail(st, err);
    ResidentSet& r = sc->resident;
    HIP_TRY(hipSetDevice(sc->device));
    sc->groups_denoised = false;
    const size_t np = (size_t)r.width * r.height, group_bytes = 16 * np * sc->groups_count;
    st = reserve_filter_buffers(r, np, {{&sc->group_den_film, 16 * np}, {&sc->group_den_var, 4 * np}, {&sc->group_dn_buf[0], group_bytes}, {&sc->group_dn_buf[1], group_bytes},
                                        {&sc->group_den_films, group_bytes}});   // (none of them zero bytes: a checked call has pixels and groups)
    if (st != PT_OK) return st;
    ptk::DnRun run = resident_filter_run(r);
    run.out_film = sc->group_den_film.as<float>(); run.out_variance = sc->group_den_var.as<float>();
    run.groups = sc->groups_count; run.group_films = sc->group_films_cache.as<float>();
    run.group_buf[0] = sc->group_dn_buf[0].as<float>(); run.group_buf[1] = sc->group_dn_buf[1].as<float>(); run.out_groups = sc->group_den_films.as<float>();
    st = run_resident_filter(d, &run, np, out_film, out_variance, out_group_films, group_bytes);
    if (st != PT_OK) return st;
    sc->groups_denoised = true;
    return PT_OK;
}
pt_status pt_spectral_project_resident_denoised(pt_scene* sc, uint32_t K, const float* matrix, float* out) {
    std::string err;
    const pt_status st = pth::check_resident_project_args(sc, K, matrix, out, resident_now(sc), &err);
    if (st != PT_OK) return fail(st, err);
    const ResidentSet& r = sc->resident;
    return project_device_bins(sc, K, matrix, r.bins, (size_t)r.width * r.height, r.denoised_bins, out);
}

pt_status pt_bsdf_sample(pt_scene* sc, uint32_t material, size_t n, const float* lambda, const float* wi, const float* s2, float* f, float* wo, float* pdf) {
    if (!sc || material >= sc->host.material_count) return fail(PT_ERR_INVALID_ARGUMENT, "bad material");
    return probe_material(sc, 0, sc->host.blob[PT_HDR_MATERIAL_OFF] + material * PT_MAT_WORDS, n, lambda, wi, 3, s2, 2, f, wo, pdf);
}
pt_status pt_light_sample(pt_scene* sc, uint32_t light_entry, size_t n, const float* from, const float* sample2d, float* dir, float* pdf) {
    if (!sc || light_entry >= sc->host.light_count) return fail(PT_ERR_INVALID_ARGUMENT, "bad light entry");
    if (n == 0) return PT_OK;
    DevBuf df, ds, dd, dp;
    HIP_TRY(df.alloc(12 * n)); HIP_TRY(ds.alloc(8 * n)); HIP_TRY(dd.alloc(12 * n)); HIP_TRY(dp.alloc(4 * n));
    HIP_TRY(hipMemcpy(df.p, from, 12 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ds.p, sample2d, 8 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_light, dim3(256), dim3(kBlock), 0, 0, sc->d_blob, sc->d_tex, light_entry, (uint32_t)n, df.as<float>(), ds.as<float>(), dd.as<float>(), dp.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dir, dd.p, 12 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pdf, dp.p, 4 * n, hipMemcpyDeviceToHost));
    return PT_OK;
}
pt_status pt_bsdf_eval(pt_scene* sc, uint32_t material, size_t n, const float* lambda, const float* wi, const float* wo, float* f, float* pdf) {
    if (!sc || material >= sc->host.material_count) return fail(PT_ERR_INVALID_ARGUMENT, "bad material");
    return probe_material(sc, 1, sc->host.blob[PT_HDR_MATERIAL_OFF] + material * PT_MAT_WORDS, n, lambda, wi, 3, wo, 3, f, nullptr, pdf);
}
pt_status pt_emission(pt_scene* sc, uint32_t material, size_t n, const float* lambda, const float* wi, float* emission) {
    if (!sc || material >= sc->host.material_count) return fail(PT_ERR_INVALID_ARGUMENT, "bad material");
    return probe_material(sc, 2, sc->host.blob[PT_HDR_MATERIAL_OFF] + material * PT_MAT_WORDS, n, lambda, wi, 3, nullptr, 0, emission, nullptr, nullptr);
}
pt_status pt_curve_eval(pt_scene* sc, uint32_t curve, size_t n, const float* lambda, float* value) {
    if (!sc || curve >= sc->host.curve_count) return fail(PT_ERR_INVALID_ARGUMENT, "bad curve");
    return probe_material(sc, 3, sc->host.curve_offsets[curve], n, lambda, nullptr, 0, nullptr, 0, value, nullptr, nullptr);
}

// Not part of pt_api.h: numeric-contract probe used by the GPU parity tests (device arithmetic vs x86).
pt_status pt_debug_numerics(int which, size_t n, const float* x, const float* y, float* out) {
    pt_status st = ensure_device();
    if (st != PT_OK) return st;
    DevBuf dx, dy, dout;
    HIP_TRY(dx.alloc(4 * n)); HIP_TRY(dy.alloc(4 * n)); HIP_TRY(dout.alloc(4 * n));
    HIP_TRY(hipMemcpy(dx.p, x, 4 * n, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dy.p, y, 4 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_numerics, dim3(256), dim3(kBlock), 0, 0, which, (uint32_t)n, dx.as<float>(), dy.as<float>(), dout.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, 4 * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Not part of pt_api.h: size of the scene blob and whether kernels read it from LDS (reported by bench.py).
uint32_t pt_debug_scene_info(pt_scene* sc, int what) {
    if (what >= 1000000) return (size_t)(what - 1000000) < sc->host.blob.size() ? sc->host.blob[(size_t)(what - 1000000)] : 0u;   // a word of the blob
    switch (what) { case 0: return sc->blob_words * 4; case 1: return (uint32_t)sc->lds_mode; case 2: return sc->host.light_count; case 3: return (uint32_t)sc->num_cus;
                    case 4: return sc->host.blob[PT_HDR_SWEEP_OFF] != 0 && !(sc->host.blob[PT_HDR_FLAGS] & PT_FLAG_NO_SWEEP) ? 1u : 0u;
                    case 7: return sc->host.blob[PT_HDR_CORE_WORDS] * 4;
                    case 9: return sc->lacks;   // PT_SCENE_* bits (1 above: lds_mode; the two answers of pth::plan_scene)
                    case 8: return (uint32_t)(sc->host.tex.size() > 0xffffffffull ? 0xffffffffull : sc->host.tex.size());   // words of texels + importance-map tables (read through L2, never staged)
                    default: return 0; }
}

}  // extern "C"
