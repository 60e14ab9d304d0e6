// pt_spectral_project.hip — developing a spectral film (include/pt_spectral.h) on gfx950: k_spectral_project, the host-array entry
// pt_spectral_project, and the host-only pt_spectral_response_matrix.  The resident entry is pt_engine.hip's (the bins are the scene's); it launches the
// same kernel.  The per-pixel rule is pt_spectral_project_rules.h's, the text the host emulation compiles.
//
// One lane per pixel, 256 lanes, grid-stride.  A lane walks the bins once, loads S_b(p) once — neighbouring lanes hold neighbouring pixels, so the load is a
// coalesced row segment of the plane — and updates KC accumulators.  KC is a template constant (1 .. 8) and the loop over k is unrolled, so the accumulators
// are registers; an array indexed by a run-time k would go to scratch.  K <= 8 reads every plane once, K <= 16 twice (8 and K - 8).
// The weights depend on (k, b) alone: they are read through a const __restrict__ kernel-argument pointer at an index made of kernel arguments and the loop
// counter, which the compiler proves uniform and turns into scalar loads (s_load_dword, one per weight and bin, shared by the 64 lanes) — no vector load, no
// LDS, no barrier.  DESIGN.md section 14 has what the compiler made of it.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pt_spectral.h"
#include "pt_error.h"
#include "pt_plan.h"
#include "pt_scene_host.h"
#include "pt_spectral_project_launch.h"
#include "pt_spectral_project_rules.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;
static_assert(SP_MAX_RESPONSES == PT_SPECTRAL_MAX_RESPONSES && SP_MAX_SUBSAMPLES == PT_SPECTRAL_MAX_SUBSAMPLES, "the rules' caps are the header's");
static_assert(SP_CIE_X == PT_RESPONSE_CIE_X && SP_CIE_Y == PT_RESPONSE_CIE_Y && SP_CIE_Z == PT_RESPONSE_CIE_Z, "the rules' constants are the header's");
static_assert(SP_MAX_RESPONSES <= 2 * SP_CHUNK, "two passes over the planes at most");

pt_status pfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }

}  // namespace

namespace ptk {
// matrix: the first of this launch's KC rows (bins floats apart); out: the first of its KC planes
template <int KC>
__global__ void __launch_bounds__(kBlock) k_spectral_project(uint32_t n_pixels, uint32_t bins, const float* __restrict__ matrix, const float* __restrict__ spectral,
                                                            float* __restrict__ out) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pixels; p += gridDim.x * blockDim.x) {
        const float* px = spectral + p;
        float* o = out + p;
        spectral_project_pixel<KC>(
            bins, [&](uint32_t b) { return px[(size_t)b * n_pixels]; }, [&](int k, uint32_t b) { return matrix[(uint32_t)k * bins + b]; },
            [&](int k, float v) { o[(size_t)k * n_pixels] = v; });
    }
}

}  // namespace ptk

namespace {

template <int KC>
void launch(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t bins, const float* matrix, const float* spectral, float* out) {
    hipLaunchKernelGGL(ptk::k_spectral_project<KC>, dim3(grid), dim3(kBlock), 0, stream, n_pixels, bins, matrix, spectral, out);
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

hipError_t launch_spectral_project(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t bins, uint32_t K, const float* matrix, const float* spectral, float* out) {
    if (K == 0 || K > (uint32_t)SP_MAX_RESPONSES || bins == 0 || bins > PT_SPECTRAL_MAX_BINS || n_pixels == 0 || n_pixels > 0x7fffffffu || grid <= 0) return hipErrorInvalidValue;
    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)SP_CHUNK) {
        const float* m = matrix + (size_t)k0 * bins;
        float* o = out + (size_t)k0 * n_pixels;
        switch (K - k0 < (uint32_t)SP_CHUNK ? K - k0 : (uint32_t)SP_CHUNK) {
            case 1: launch<1>(grid, stream, n_pixels, bins, m, spectral, o); break;
            case 2: launch<2>(grid, stream, n_pixels, bins, m, spectral, o); break;
            case 3: launch<3>(grid, stream, n_pixels, bins, m, spectral, o); break;
            case 4: launch<4>(grid, stream, n_pixels, bins, m, spectral, o); break;
            case 5: launch<5>(grid, stream, n_pixels, bins, m, spectral, o); break;
            case 6: launch<6>(grid, stream, n_pixels, bins, m, spectral, o); break;
            case 7: launch<7>(grid, stream, n_pixels, bins, m, spectral, o); break;
            default: launch<8>(grid, stream, n_pixels, bins, m, spectral, o); break;
        }
    }
    return hipGetLastError();
}

}  // namespace ptk

extern "C" pt_status pt_spectral_response_matrix(const pt_render_desc* rd, const pt_spectral_desc* sd, const pt_curve* curves, uint32_t curve_count, const float* curve_data,
                                                 uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, float* matrix) {
    std::string err;
    const pt_status st = pth::check_response_matrix_args(rd, sd, curves, curve_count, curve_data, curve_data_floats, K, responses, filter, subsamples, matrix, &err);
    if (st != PT_OK) return pfail(st, err);
    if (!pth::spectral_response_matrix(rd->wavelength_lo, rd->wavelength_hi, sd->bins, curves, curve_count, curve_data, curve_data_floats, K, responses, filter, subsamples,
                                       matrix, &err))
        return pfail(PT_ERR_INVALID_ARGUMENT, err);
    return PT_OK;
}

extern "C" pt_status pt_spectral_project(uint32_t width, uint32_t height, uint32_t bins, uint32_t K, const float* matrix, const float* spectral, float* out) {
    std::string err;
    const pt_status st = pth::check_spectral_project_args(width, height, bins, K, matrix, spectral, out, &err);
    if (st != PT_OK) return pfail(st, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return pfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
#define SP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return pfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    SP_TRY(hipSetDevice(0));
    int cus = 0;
    SP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const size_t np = (size_t)width * height;
    Dev d_matrix, d_bins, d_out;
    SP_TRY(d_matrix.alloc(sizeof(float) * K * bins)); SP_TRY(d_bins.alloc(sizeof(float) * bins * np)); SP_TRY(d_out.alloc(sizeof(float) * K * np));
    SP_TRY(hipMemcpy(d_matrix.p, matrix, sizeof(float) * K * bins, hipMemcpyHostToDevice));
    SP_TRY(hipMemcpy(d_bins.p, spectral, sizeof(float) * bins * np, hipMemcpyHostToDevice));
    SP_TRY(ptk::launch_spectral_project(ptk::spectral_project_grid(cus, (uint32_t)np), nullptr, (uint32_t)np, bins, K, d_matrix.as<float>(), d_bins.as<float>(), d_out.as<float>()));
    SP_TRY(hipDeviceSynchronize());
    SP_TRY(hipMemcpy(out, d_out.p, sizeof(float) * K * np, hipMemcpyDeviceToHost));
#undef SP_TRY
    return PT_OK;
}
