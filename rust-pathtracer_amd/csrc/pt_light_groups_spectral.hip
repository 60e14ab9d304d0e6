// pt_light_groups_spectral.hip — spectral light groups (include/pt_light_groups_spectral.h) on gfx950: k_accumulate_group_bins, the
// wavelength-binned film of every light group, k_light_groups_relamp, the re-lamp, the host-array entry pt_light_groups_relamp and the host-only
// pt_light_groups_relamp_matrix.  The render and the resident entries are pt_engine.hip's (the bins are the scene's); they launch the same kernels.  The
// per-pixel rules are pt_light_groups_spectral_rules.h's and pt_spectral_project_rules.h's, the text the host emulation compiles.
//
// k_accumulate_group_bins is k_accumulate_spectral's sibling: one lane per pixel of the pass and group, the group in blockIdx.y as in k_accumulate_groups, so
// that a wave's lanes hold neighbouring pixels of one tile row and every load and store of a plane coalesces.  A lane needs `bins` accumulators indexed by a
// value known only at run time; they live in its column of LDS, bin b of lane t at lds[b * blockDim.x + t].  The bank is a function of the lane alone — no
// conflicts whatever the bins are — and a lane touches only its own column, so there is no barrier (lanes leave the grid-stride loop at different trip
// counts).  A pixel continued by a later pass starts from the value the earlier pass stored: the passes' accumulate steps are ordered by the pass loop.
//
// k_light_groups_relamp: spectral_project_pixel<KC> over G * bins <= 512 planes.  One lane per pixel, 256 lanes, grid-stride; the KC accumulators are registers
// (KC a template constant, the loop over k unrolled); the weights depend on (k, plane) alone and are read through a const __restrict__ kernel-argument pointer
// at an index made of kernel arguments and the loop counter, which the compiler proves uniform and turns into scalar loads shared by the 64 lanes — no vector
// load, no LDS, no barrier.  K <= 8 reads every plane once, K <= 16 twice (8 and K - 8).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pt_light_groups_spectral.h"
#include "pt_error.h"
#include "pt_light_groups_spectral_launch.h"
#include "pt_light_groups_spectral_rules.h"
#include "pt_plan.h"
#include "pt_scene_host.h"
#include "pt_spectral_project_launch.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxLdsBytes = kBlock * PT_SPECTRAL_MAX_BINS * sizeof(float);   // 64 KB
static_assert(LGS_KEEP == PT_RELAMP_KEEP, "the rules' constant is the header's");
static_assert(LGS_MAX_PLANES == PT_LIGHT_GROUPS_MAX * PT_SPECTRAL_MAX_BINS, "the rules' cap is the headers'");
static_assert(SP_MAX_RESPONSES <= 2 * SP_CHUNK, "two passes over the planes at most");

pt_status pfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }

__global__ void __launch_bounds__(kBlock) k_accumulate_group_bins(RenderParams rp, const uint32_t* __restrict__ pixels, const float* __restrict__ energy,
                                                                 float* __restrict__ group_spectral, uint32_t bins, uint32_t plane_pixels) {
    extern __shared__ float lds[];
    float* col = lds + threadIdx.x;
    const uint32_t step = blockDim.x, group = blockIdx.y;
    float* planes = group_spectral + (size_t)group * bins * plane_pixels;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < rp.chunk_pixels; p += gridDim.x * blockDim.x) {
        float* px = planes + pixels[p];   // (neighbouring lanes hold neighbouring pixels of a tile row: each plane's loads and stores coalesce)
        for (uint32_t b = 0; b < bins; ++b) col[b * step] = px[(size_t)b * plane_pixels];
        lg_spectral_fold_pixel(rp, bins, energy, group, p, [&](uint32_t b) -> float& { return col[b * step]; });
        for (uint32_t b = 0; b < bins; ++b) px[(size_t)b * plane_pixels] = col[b * step];
    }
}

// matrix: the first of this launch's KC rows (planes floats apart); out: the first of its KC planes
template <int KC>
__global__ void __launch_bounds__(kBlock) k_light_groups_relamp(uint32_t n_pixels, uint32_t planes, const float* __restrict__ matrix, const float* __restrict__ group_spectral,
                                                               float* __restrict__ out) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += gridDim.x * blockDim.x) {
        const float* px = group_spectral + p;
        float* o = out + p;
        spectral_project_pixel<KC>(
            planes, [&](uint32_t i) { return px[(size_t)i * n_pixels]; }, [&](int k, uint32_t i) { return matrix[(uint32_t)k * planes + i]; },
            [&](int k, float v) { o[(size_t)k * n_pixels] = v; });
    }
}

template <int KC>
void launch_relamp(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t planes, const float* matrix, const float* group_spectral, float* out) {
    hipLaunchKernelGGL(k_light_groups_relamp<KC>, dim3(grid), dim3(kBlock), 0, stream, n_pixels, planes, matrix, group_spectral, out);
}

// one workgroup per 256 items, at most 16384 (the grid-stride loop takes the rest)
int lanes_grid(uint32_t items) {
    const uint32_t need = (items + (uint32_t)kBlock - 1u) / (uint32_t)kBlock;
    return (int)(need < 16384u ? (need ? need : 1u) : 16384u);
}

struct Dev {
    void* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

namespace ptk {

hipError_t launch_accumulate_group_bins(hipStream_t stream, const RenderParams& rp, const uint32_t* pixels, const float* energy, float* group_spectral,
                                        uint32_t group_count, uint32_t bins, uint32_t plane_pixels) {
    if (group_count == 0 || group_count > LG_MAX_GROUPS || bins == 0 || bins > PT_SPECTRAL_MAX_BINS || !group_spectral || plane_pixels == 0 || plane_pixels > 0x7fffffffu)
        return hipErrorInvalidValue;
    // (64 KB at 64 bins: above the 48 KB a kernel may take without asking; per launch, because the attribute belongs to the current device)
    const hipError_t allowed = hipFuncSetAttribute(reinterpret_cast<const void*>(k_accumulate_group_bins), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
    if (allowed != hipSuccess) return allowed;
    hipLaunchKernelGGL(k_accumulate_group_bins, dim3(lanes_grid(rp.chunk_pixels), group_count), dim3(kBlock), (size_t)kBlock * bins * sizeof(float), stream, rp, pixels,
                       energy, group_spectral, bins, plane_pixels);
    return hipGetLastError();
}

hipError_t launch_light_groups_relamp(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t planes, uint32_t K, const float* matrix, const float* group_spectral,
                                      float* out) {
    if (K == 0 || K > (uint32_t)SP_MAX_RESPONSES || planes == 0 || planes > LGS_MAX_PLANES || n_pixels == 0 || n_pixels > 0x7fffffffu || grid <= 0) return hipErrorInvalidValue;
    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)SP_CHUNK) {
        const float* m = matrix + (size_t)k0 * planes;
        float* o = out + (size_t)k0 * n_pixels;
        switch (K - k0 < (uint32_t)SP_CHUNK ? K - k0 : (uint32_t)SP_CHUNK) {
            case 1: launch_relamp<1>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            case 2: launch_relamp<2>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            case 3: launch_relamp<3>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            case 4: launch_relamp<4>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            case 5: launch_relamp<5>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            case 6: launch_relamp<6>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            case 7: launch_relamp<7>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
            default: launch_relamp<8>(grid, stream, n_pixels, planes, m, group_spectral, o); break;
        }
    }
    return hipGetLastError();
}

}  // namespace ptk

extern "C" pt_status pt_light_groups_relamp_matrix(const pt_render_desc* rd, const pt_spectral_desc* sd, const pt_curve* curves, uint32_t curve_count, const float* curve_data,
                                                   uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples,
                                                   uint32_t group_count, const int32_t* old_curve, const int32_t* new_curve, const float* gain, float* matrix) {
    std::string err;
    const pt_status st = pth::light_groups_relamp_matrix(rd, sd, curves, curve_count, curve_data, curve_data_floats, K, responses, filter, subsamples, group_count, old_curve,
                                                         new_curve, gain, matrix, &err);
    if (st != PT_OK) return pfail(st, err);
    return PT_OK;
}

extern "C" pt_status pt_light_groups_relamp(uint32_t width, uint32_t height, uint32_t group_count, uint32_t bins, uint32_t K, const float* matrix,
                                            const float* group_spectral, float* out) {
    std::string err;
    const pt_status st = pth::check_relamp_args(width, height, group_count, bins, K, matrix, group_spectral, out, &err);
    if (st != PT_OK) return pfail(st, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return pfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
#define LGS_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return pfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    LGS_TRY(hipSetDevice(0));
    int cus = 0;
    LGS_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const size_t np = (size_t)width * height;
    const uint32_t planes = group_count * bins;
    Dev d_matrix, d_bins, d_out;
    LGS_TRY(d_matrix.alloc(sizeof(float) * K * planes)); LGS_TRY(d_bins.alloc(sizeof(float) * planes * np)); LGS_TRY(d_out.alloc(sizeof(float) * K * np));
    LGS_TRY(hipMemcpy(d_matrix.p, matrix, sizeof(float) * K * planes, hipMemcpyHostToDevice));
    LGS_TRY(hipMemcpy(d_bins.p, group_spectral, sizeof(float) * planes * np, hipMemcpyHostToDevice));
    LGS_TRY(ptk::launch_light_groups_relamp(ptk::spectral_project_grid(cus, (uint32_t)np), nullptr, (uint32_t)np, planes, K, d_matrix.as<float>(), d_bins.as<float>(), d_out.as<float>()));
    LGS_TRY(hipDeviceSynchronize());
    LGS_TRY(hipMemcpy(out, d_out.p, sizeof(float) * K * np, hipMemcpyDeviceToHost));
#undef LGS_TRY
    return PT_OK;
}
