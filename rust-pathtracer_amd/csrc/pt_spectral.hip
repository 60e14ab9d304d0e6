// pt_spectral.hip — the wavelength-binned film of include/pt_spectral.h on gfx950: k_accumulate_spectral, a second accumulate
// kernel over the energy planes k_accumulate has just read, and the host-only pt_spectral_bin_centres.  The per-sample rule is pt_spectral_rules.h's,
// the text the host emulation compiles.
//
// A lane owns one pixel of the pass and needs `bins` accumulators indexed by a value known only at run time.  A register array indexed that way goes
// to scratch, and a read-modify-write of global memory per sample is a dependent chain of HBM round trips, so the accumulators live in LDS: bin b of
// lane t at lds[b * blockDim.x + t].  The bank is then a function of the lane alone — no conflicts whatever the bins are — and a lane touches only its
// own column, so the kernel has no barrier (lanes leave the grid-stride loop at different trip counts).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pt_spectral.h"
#include "pt_error.h"
#include "pt_plan.h"
#include "pt_spectral_launch.h"
#include "pt_spectral_rules.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxLdsBytes = kBlock * PT_SPECTRAL_MAX_BINS * sizeof(float);   // 64 KB

template <int NL>
__global__ void __launch_bounds__(kBlock) k_accumulate_spectral(RenderParams rp, const uint32_t* __restrict__ pixels, const float* __restrict__ energy,
                                                               float* __restrict__ spectral, uint32_t bins, uint32_t plane_pixels) {
    extern __shared__ float lds[];
    float* col = lds + threadIdx.x;
    const uint32_t step = blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < rp.chunk_pixels; p += gridDim.x * blockDim.x) {
        const uint32_t pixel = pixels[p];
        float* px = spectral + pixel;   // (neighbouring lanes hold neighbouring pixels of a tile row: each plane's loads and stores coalesce)
        for (uint32_t b = 0; b < bins; ++b) col[b * step] = px[(size_t)b * plane_pixels];
        spectral_fold_pixel<NL>(rp, bins, energy, p, pixel, [&](uint32_t b) -> float& { return col[b * step]; });
        for (uint32_t b = 0; b < bins; ++b) px[(size_t)b * plane_pixels] = col[b * step];
    }
}

template <int NL>
hipError_t launch(int grid, hipStream_t stream, const RenderParams& rp, const uint32_t* pixels, const float* energy, float* spectral, uint32_t bins, uint32_t plane_pixels) {
    // (64 KB at 64 bins: above the 48 KB a kernel may take without asking; per launch, because the attribute belongs to the current device)
    const hipError_t allowed = hipFuncSetAttribute(reinterpret_cast<const void*>(k_accumulate_spectral<NL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
    if (allowed != hipSuccess) return allowed;
    hipLaunchKernelGGL(k_accumulate_spectral<NL>, dim3(grid), dim3(kBlock), (size_t)kBlock * bins * sizeof(float), stream, rp, pixels, energy, spectral, bins, plane_pixels);
    return hipSuccess;
}

}  // namespace

namespace ptk {

hipError_t launch_accumulate_spectral(int nl, int grid, hipStream_t stream, const RenderParams& rp, const uint32_t* pixels, const float* energy, float* spectral,
                                      uint32_t bins, uint32_t plane_pixels) {
    if (bins == 0 || bins > PT_SPECTRAL_MAX_BINS || grid <= 0) return hipErrorInvalidValue;
    return nl == 4 ? launch<4>(grid, stream, rp, pixels, energy, spectral, bins, plane_pixels) : launch<1>(grid, stream, rp, pixels, energy, spectral, bins, plane_pixels);
}

}  // namespace ptk

extern "C" pt_status pt_spectral_bin_centres(const pt_render_desc* rd, const pt_spectral_desc* sd, float* centres_nm) {
    std::string err;
    const pt_status st = pth::spectral_bin_centres(rd, sd, centres_nm, &err);
    if (st != PT_OK) pt_set_error(err);
    return st;
}
