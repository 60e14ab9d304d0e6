// pt_light_groups.hip — the films of a light-group render (include/pt_light_groups.h) on gfx950: k_accumulate_groups, k_accumulate over
// the group planes of a pass's energy buffer, k_adaptive_finish_groups, the division of an adaptive group render's running sums, k_light_groups_mix, the relight, and the host-array entry pt_light_groups_mix.  The render and the resident
// entries are pt_engine.hip's (the films are the scene's); they launch the same kernels.  The per-pixel rules are pt_light_group_rules.h's, the text the host
// emulation compiles.
//
// k_accumulate_groups: one lane per pixel of the pass and group, the group in blockIdx.y, so that a wave's lanes hold neighbouring pixels of one plane and
// every load of a plane and every float4 of a film coalesces, as in k_accumulate.
// k_light_groups_mix: one lane per pixel, grid-stride.  A lane makes one 16-byte load per group and one 16-byte store.  The matrices depend on g alone: they
// are read through a const __restrict__ kernel-argument pointer at an index made of the loop counter, which the compiler proves uniform and turns into scalar
// loads shared by the 64 lanes — no vector load, no LDS, no barrier.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pt_light_groups.h"
#include "pt_error.h"
#include "pt_light_groups_launch.h"
#include "pt_plan.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;
static_assert(LG_MAX_GROUPS == PT_LIGHT_GROUPS_MAX, "the rules' cap is the header's");

pt_status pfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }

__global__ void __launch_bounds__(kBlock) k_accumulate_groups(RenderParams rp, const uint32_t* __restrict__ pixels, const float* __restrict__ energy,
                                                             float* __restrict__ group_films, size_t film_pixels) {
    const uint32_t group = blockIdx.y;
    float4* film = reinterpret_cast<float4*>(group_films) + (size_t)group * film_pixels;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < rp.chunk_pixels; p += gridDim.x * blockDim.x) {
        const uint32_t pixel = pixels[p];
        float4* px = film + pixel;
        const float4 v = *px;
        float f[4] = {v.x, v.y, v.z, v.w};
        lg_accumulate_pixel(rp, energy, group, p, pixel, f);
        *px = make_float4(f[0], f[1], f[2], f[3]);
    }
}

__global__ void __launch_bounds__(kBlock) k_light_groups_mix(uint32_t n_pixels, uint32_t group_count, const float* __restrict__ group_films,
                                                            const float* __restrict__ matrices, float* __restrict__ out) {
    const float4* films = reinterpret_cast<const float4*>(group_films);
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += gridDim.x * blockDim.x) {
        float o[4];
        lg_mix_pixel(group_count, matrices, [&](uint32_t g, float* x, float* y, float* z) { const float4 v = films[(size_t)g * n_pixels + p]; *x = v.x; *y = v.y; *z = v.z; }, o);
        reinterpret_cast<float4*>(out)[p] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// the finish of an adaptive group render: one lane per pixel and group, the group in blockIdx.y as in k_accumulate_groups; a lane reads its pixel's count and
// makes one 16-byte load and store (lg_adaptive_finish_pixel)
__global__ void __launch_bounds__(kBlock) k_adaptive_finish_groups(uint32_t n_pixels, const uint32_t* __restrict__ counts, float* __restrict__ group_films) {
    float4* film = reinterpret_cast<float4*>(group_films) + (size_t)blockIdx.y * n_pixels;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += gridDim.x * blockDim.x) {
        const uint32_t n = counts[p];
        if (n == 0u) continue;
        const float4 v = film[p];
        float f[4] = {v.x, v.y, v.z, v.w};
        lg_adaptive_finish_pixel(n, f);
        film[p] = make_float4(f[0], f[1], f[2], f[3]);
    }
}

// one workgroup per 256 items, at most 16384 (the grid-stride loops take the rest)
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

hipError_t launch_accumulate_groups(hipStream_t stream, const RenderParams& rp, const uint32_t* pixels, const float* energy, float* group_films, uint32_t group_count,
                                    size_t film_pixels) {
    if (group_count == 0 || group_count > LG_MAX_GROUPS || !group_films) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accumulate_groups, dim3(lanes_grid(rp.chunk_pixels), group_count), dim3(kBlock), 0, stream, rp, pixels, energy, group_films, film_pixels);
    return hipGetLastError();
}

hipError_t launch_adaptive_finish_groups(hipStream_t stream, uint32_t n_pixels, const uint32_t* counts, float* group_films, uint32_t group_count) {
    if (group_count == 0 || group_count > LG_MAX_GROUPS || !group_films || !counts || n_pixels == 0 || n_pixels > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_adaptive_finish_groups, dim3(lanes_grid(n_pixels), group_count), dim3(kBlock), 0, stream, n_pixels, counts, group_films);
    return hipGetLastError();
}

hipError_t launch_light_groups_mix(hipStream_t stream, uint32_t n_pixels, uint32_t group_count, const float* group_films, const float* matrices, float* out) {
    if (group_count == 0 || group_count > LG_MAX_GROUPS || n_pixels == 0 || n_pixels > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_light_groups_mix, dim3(lanes_grid(n_pixels)), dim3(kBlock), 0, stream, n_pixels, group_count, group_films, matrices, out);
    return hipGetLastError();
}

}  // namespace ptk

extern "C" pt_status pt_light_groups_mix(uint32_t width, uint32_t height, uint32_t group_count, const float* group_films, const float* matrices, float* out_xyzw) {
    std::string err;
    const pt_status st = pth::check_light_groups_mix_args(width, height, group_count, group_films, matrices, out_xyzw, &err);
    if (st != PT_OK) return pfail(st, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return pfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
#define LG_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return pfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    LG_TRY(hipSetDevice(0));
    const size_t np = (size_t)width * height, film_bytes = sizeof(float) * 4 * np;
    Dev d_matrices, d_films, d_out;
    LG_TRY(d_matrices.alloc(sizeof(float) * 9 * group_count)); LG_TRY(d_films.alloc(film_bytes * group_count)); LG_TRY(d_out.alloc(film_bytes));
    LG_TRY(hipMemcpy(d_matrices.p, matrices, sizeof(float) * 9 * group_count, hipMemcpyHostToDevice));
    LG_TRY(hipMemcpy(d_films.p, group_films, film_bytes * group_count, hipMemcpyHostToDevice));
    LG_TRY(ptk::launch_light_groups_mix(nullptr, (uint32_t)np, group_count, d_films.as<float>(), d_matrices.as<float>(), d_out.as<float>()));
    LG_TRY(hipDeviceSynchronize());
    LG_TRY(hipMemcpy(out_xyzw, d_out.p, film_bytes, hipMemcpyDeviceToHost));
#undef LG_TRY
    return PT_OK;
}
