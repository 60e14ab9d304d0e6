// pt_shard.hip — a shard's planes in packed form on gfx950: the spectral film (include/pt_spectral.h) in floats and the group films
// (include/pt_light_groups_multi.h, DESIGN.md section 15 "On every device of a node") in pixels of four floats.  k_spectral_pack and k_light_groups_pack are what
// the node entries (pt_render_spectral_multi, pt_render_light_groups_multi and their adaptive forms, pt_engine.hip) run on every device behind its render;
// their inverses k_spectral_unpack and k_light_groups_unpack are what pt_resident_assemble (include/pt_resident.h) runs once per shard on the device that
// filters.  The index rule is pt_shard_rules.h's, the text the host scatter and the host emulation compile.
//
// One lane per item of the shard's pixel list, 256 lanes, grid-stride.  A lane loads px[i] once and walks the planes: one load and one store of an element per
// plane.  Neighbouring lanes hold neighbouring pixels of a tile row, so a wave's load of one plane is two runs of 32 pixels (128 bytes each in floats, 512 in
// pixels) and its store 256 (1024) contiguous bytes.  No LDS, no barrier, no atomics: the kernel moves n_own * (4 + 8 * planes) bytes in floats,
// n_own * (4 + 32 * planes) in pixels, and does nothing else.  The unpack is the same walk with load and store exchanged.
//
// The four kernels keep their names (the profiles and the tools' --summarise modes select dispatches by them): each is one call of the loop, written once.
// The kernel reads blockDim.x and hands it to the loop as `block`: read inside the device template the compiler keeps the general form of that read (a
// choice between the group size and the remainder of a non-uniform grid, loaded per lane), read in the kernel it is one scalar load.
#include <hip/hip_runtime.h>

#include "../../include/pt_light_groups.h"
#include "../../include/pt_spectral.h"
#include "pt_shard_launch.h"
#include "pt_shard_rules.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;

template <typename Q>
__device__ __forceinline__ void pack_loop(const Q* __restrict__ full, uint32_t full_pixels, const uint32_t* __restrict__ px, uint32_t n_own, uint32_t planes,
                                          Q* __restrict__ packed, uint32_t block) {
    // (64-bit: n_own may be within a grid's stride of 2^32)
    for (size_t i = (size_t)blockIdx.x * block + threadIdx.x; i < n_own; i += (size_t)gridDim.x * block)
        shard_pack_item(full, full_pixels, px, n_own, planes, (uint32_t)i, packed);
}
template <typename Q>
__device__ __forceinline__ void unpack_loop(const Q* __restrict__ packed, const uint32_t* __restrict__ px, uint32_t n_own, uint32_t planes, Q* __restrict__ full,
                                            uint32_t full_pixels, uint32_t block) {
    for (size_t i = (size_t)blockIdx.x * block + threadIdx.x; i < n_own; i += (size_t)gridDim.x * block)
        shard_unpack_item(packed, px, n_own, planes, (uint32_t)i, full, full_pixels);
}

__global__ void __launch_bounds__(kBlock) k_spectral_pack(const float* __restrict__ full, uint32_t full_pixels, const uint32_t* __restrict__ px, uint32_t n_own,
                                                         uint32_t planes, float* __restrict__ packed) { pack_loop(full, full_pixels, px, n_own, planes, packed, blockDim.x); }
__global__ void __launch_bounds__(kBlock) k_spectral_unpack(const float* __restrict__ packed, const uint32_t* __restrict__ px, uint32_t n_own, uint32_t planes,
                                                           float* __restrict__ full, uint32_t full_pixels) { unpack_loop(packed, px, n_own, planes, full, full_pixels, blockDim.x); }
__global__ void __launch_bounds__(kBlock) k_light_groups_pack(const float4* __restrict__ full, uint32_t full_pixels, const uint32_t* __restrict__ px, uint32_t n_own,
                                                             uint32_t planes, float4* __restrict__ packed) { pack_loop(full, full_pixels, px, n_own, planes, packed, blockDim.x); }
__global__ void __launch_bounds__(kBlock) k_light_groups_unpack(const float4* __restrict__ packed, const uint32_t* __restrict__ px, uint32_t n_own, uint32_t planes,
                                                               float4* __restrict__ full, uint32_t full_pixels) { unpack_loop(packed, px, n_own, planes, full, full_pixels, blockDim.x); }

bool refused(uint32_t elem_floats, int grid, const void* full, uint32_t full_pixels, const void* px, uint32_t n_own, uint32_t planes, const void* packed) {
    if (elem_floats != 1 && elem_floats != 4) return true;
    const uint32_t cap = elem_floats == 1 ? PT_SPECTRAL_MAX_BINS : PT_LIGHT_GROUPS_MAX;
    return planes == 0 || planes > cap || n_own == 0 || n_own > full_pixels || grid <= 0 || !full || !px || !packed;
}

}  // namespace

namespace ptk {

hipError_t launch_shard_pack(uint32_t elem_floats, int grid, hipStream_t stream, const float* full, uint32_t full_pixels, const uint32_t* px, uint32_t n_own, uint32_t planes,
                             float* packed) {
    if (refused(elem_floats, grid, full, full_pixels, px, n_own, planes, packed)) return hipErrorInvalidValue;
    if (elem_floats == 1) hipLaunchKernelGGL(k_spectral_pack, dim3(grid), dim3(kBlock), 0, stream, full, full_pixels, px, n_own, planes, packed);
    else hipLaunchKernelGGL(k_light_groups_pack, dim3(grid), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(full), full_pixels, px, n_own, planes,
                            reinterpret_cast<float4*>(packed));
    return hipGetLastError();
}

hipError_t launch_shard_unpack(uint32_t elem_floats, int grid, hipStream_t stream, const float* packed, const uint32_t* px, uint32_t n_own, uint32_t planes, float* full,
                               uint32_t full_pixels) {
    if (refused(elem_floats, grid, full, full_pixels, px, n_own, planes, packed)) return hipErrorInvalidValue;
    if (elem_floats == 1) hipLaunchKernelGGL(k_spectral_unpack, dim3(grid), dim3(kBlock), 0, stream, packed, px, n_own, planes, full, full_pixels);
    else hipLaunchKernelGGL(k_light_groups_unpack, dim3(grid), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(packed), px, n_own, planes,
                            reinterpret_cast<float4*>(full), full_pixels);
    return hipGetLastError();
}

}  // namespace ptk
