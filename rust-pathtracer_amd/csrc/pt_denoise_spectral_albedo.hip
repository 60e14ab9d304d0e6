// pt_denoise_spectral_albedo.hip — the per-bin albedo guide's kernels (pt_render_guides_bin_albedo of include/pt_spectral.h, DESIGN.md section 14,
// "Demodulating the bins") on gfx950, and nothing else: the filter that demodulates the bins by this guide is pt_denoise.hip's.
//
// k_bin_albedo_tables is k_albedo_tables over rows x bins with the bins' centre wavelengths; k_guide_fold_bins folds one guide sample's first-hit records
// into the bin-major sums (launched behind k_guide_fold_albedo, which keeps the guide sum and the XYZ albedo sum as it always did; the chain folds the same
// way inside k_chain_step); k_bin_albedo_finish divides by K.  Every per-pixel rule is pt_denoise_spectral_albedo_rules.h's, the text the host emulation
// compiles, so the outputs agree with it bit for bit.
#include <hip/hip_runtime.h>

#include "pt_bin_albedo_device.h"
#include "pt_denoise_spectral_albedo_launch.h"
#include "pt_denoise_spectral_albedo_rules.h"
#include "pt_device.h"

using namespace ptd;

namespace {

constexpr int kLine = 256;

inline uint32_t line_grid(size_t n) { return (uint32_t)((n + kLine - 1) / kLine); }

// one lane per (texture layer of a Lambertian material, bin): the layer's curves at the bin's centre wavelength
__global__ void __launch_bounds__(kLine) k_bin_albedo_tables(const uint32_t* __restrict__ blob, const float* __restrict__ tex, float lo, float width, uint32_t bins, uint32_t rows,
                                                            const uint32_t* __restrict__ layer_off, float4* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * bins) return;   // (rows x bins: at most the scene's layers x 64)
    const SceneView s{blob, tex, blob + blob[PT_HDR_CORE_WORDS]};
    const LayerCurves c = layer_curves(s, layer_off[i / bins], dn_bin_centre(lo, width, i % bins));
    table[i] = make_float4(c.c0, c.c1, c.c2, c.c3);
}
__global__ void __launch_bounds__(kLine) k_guide_fold_bins(uint32_t n, const pt_hit* __restrict__ hits, ptk::BinAlbedoFold F, const uint32_t* __restrict__ blob,
                                                          const float* __restrict__ tex, uint32_t material_count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ptk::bin_albedo_fold_hit(F, i, hits[i], blob, tex, material_count);
}
// over bins x n_pixels values; bin_albedo may be sums (a lane reads and writes its own value)
__global__ void __launch_bounds__(kLine) k_bin_albedo_finish(size_t n, const float* sums, uint32_t samples, float* bin_albedo) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bin_albedo[i] = dn_bin_albedo_finish(sums[i], samples);
}

}  // namespace

namespace ptk {

void launch_bin_albedo_tables(const uint32_t* blob, const float* tex, float wavelength_lo, float bin_width, uint32_t bins, uint32_t rows, const uint32_t* layer_off, float* table) {
    if (rows == 0) return;
    hipLaunchKernelGGL(k_bin_albedo_tables, dim3(line_grid((size_t)rows * bins)), dim3(kLine), 0, 0, blob, tex, wavelength_lo, bin_width, bins, rows, layer_off,
                       reinterpret_cast<float4*>(table));
}
void launch_guide_fold_bins(uint32_t n_pixels, const pt_hit* hits, const BinAlbedoFold& fold, const uint32_t* blob, const float* tex, uint32_t material_count) {
    hipLaunchKernelGGL(k_guide_fold_bins, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, hits, fold, blob, tex, material_count);
}
void launch_bin_albedo_finish(uint32_t n_pixels, uint32_t bins, const float* sums, uint32_t samples, float* bin_albedo) {
    const size_t total = (size_t)bins * n_pixels;
    hipLaunchKernelGGL(k_bin_albedo_finish, dim3(line_grid(total)), dim3(kLine), 0, 0, total, sums, samples, bin_albedo);
}

}  // namespace ptk
