// pt_spectral_shard.hip — a shard's spectral film in packed form (include/pt_spectral.h) on gfx950: k_spectral_pack, which the node
// entries pt_render_spectral_multi and pt_render_adaptive_spectral_multi (pt_engine.hip) run on every device behind its render, and its inverse
// k_spectral_unpack, which pt_resident_assemble (include/pt_resident.h) runs once per shard on the device that filters.  The index rule is
// pt_spectral_shard_rules.h's, the text the host scatter and the host emulation compile.
//
// One lane per item of the shard's pixel list, 256 lanes, grid-stride.  A lane loads px[i] once and walks the bins.  Neighbouring lanes hold neighbouring
// pixels of a tile row, so a wave's load of one plane is two runs of 32 pixels (128 bytes each) and its store 256 contiguous bytes.  No LDS, no barrier, no
// atomics: the kernel moves n_own * (4 + 8 * bins) bytes and does nothing else.  The unpack is the same walk with load and store exchanged: a wave loads 256
// contiguous bytes of a packed plane and stores two runs of 128 bytes of a tile row.
#include <hip/hip_runtime.h>

#include "../../include/pt_spectral.h"
#include "pt_spectral_shard_launch.h"
#include "pt_spectral_shard_rules.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_spectral_pack(const float* __restrict__ planes, uint32_t plane_pixels, const uint32_t* __restrict__ px, uint32_t n_own,
                                                         uint32_t bins, float* __restrict__ packed) {
    // (64-bit: n_own may be within a grid's stride of 2^32)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_own; i += (size_t)gridDim.x * blockDim.x)
        spectral_shard_pack_item(planes, plane_pixels, px, n_own, bins, (uint32_t)i, packed);
}

__global__ void __launch_bounds__(kBlock) k_spectral_unpack(const float* __restrict__ packed, const uint32_t* __restrict__ px, uint32_t n_own, uint32_t bins,
                                                           float* __restrict__ planes, uint32_t plane_pixels) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_own; i += (size_t)gridDim.x * blockDim.x)
        spectral_shard_unpack_item(packed, px, n_own, bins, (uint32_t)i, planes, plane_pixels);
}

}  // namespace

namespace ptk {

hipError_t launch_spectral_pack(int grid, hipStream_t stream, const float* planes, uint32_t plane_pixels, const uint32_t* px, uint32_t n_own, uint32_t bins, float* packed) {
    if (bins == 0 || bins > PT_SPECTRAL_MAX_BINS || n_own == 0 || n_own > plane_pixels || grid <= 0 || !planes || !px || !packed) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spectral_pack, dim3(grid), dim3(kBlock), 0, stream, planes, plane_pixels, px, n_own, bins, packed);
    return hipGetLastError();
}

hipError_t launch_spectral_unpack(int grid, hipStream_t stream, const float* packed, const uint32_t* px, uint32_t n_own, uint32_t bins, float* planes, uint32_t plane_pixels) {
    if (bins == 0 || bins > PT_SPECTRAL_MAX_BINS || n_own == 0 || n_own > plane_pixels || grid <= 0 || !planes || !px || !packed) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spectral_unpack, dim3(grid), dim3(kBlock), 0, stream, packed, px, n_own, bins, planes, plane_pixels);
    return hipGetLastError();
}

}  // namespace ptk
