// pt_light_groups_shard.hip — a shard's group films in packed form (include/pt_light_groups_multi.h, DESIGN.md section 15 "On every device of a node") on
// gfx950: k_light_groups_pack, which the node entries pt_render_light_groups_multi and pt_render_adaptive_light_groups_multi (pt_engine.hip) run on every
// device behind its render, and its inverse k_light_groups_unpack, which pt_resident_assemble (include/pt_resident.h) runs once per shard on the device that
// filters.  The index rule is pt_light_groups_shard_rules.h's, the text the host scatter and the host emulation compile.
//
// One lane per item of the shard's pixel list, 256 lanes, grid-stride.  A lane loads px[i] once and walks the groups: one 16-byte load and one 16-byte store
// per group.  Neighbouring lanes hold neighbouring pixels of a tile row, so a wave's load of one group is two runs of 32 pixels (512 bytes each) and its
// store 1024 contiguous bytes.  No LDS, no barrier, no atomics: the kernel moves n_own * (4 + 32 * groups) bytes and does nothing else.  The unpack is the
// same walk with load and store exchanged.
#include <hip/hip_runtime.h>

#include "../../include/pt_light_groups.h"
#include "pt_light_groups_shard_launch.h"
#include "pt_light_groups_shard_rules.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_light_groups_pack(const float4* __restrict__ group_films, uint32_t film_pixels, const uint32_t* __restrict__ px,
                                                             uint32_t n_own, uint32_t groups, float4* __restrict__ packed) {
    // (64-bit: n_own may be within a grid's stride of 2^32)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_own; i += (size_t)gridDim.x * blockDim.x)
        lg_shard_pack_item(group_films, film_pixels, px, n_own, groups, (uint32_t)i, packed);
}

__global__ void __launch_bounds__(kBlock) k_light_groups_unpack(const float4* __restrict__ packed, const uint32_t* __restrict__ px, uint32_t n_own, uint32_t groups,
                                                               float4* __restrict__ group_films, uint32_t film_pixels) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_own; i += (size_t)gridDim.x * blockDim.x)
        lg_shard_unpack_item(packed, px, n_own, groups, (uint32_t)i, group_films, film_pixels);
}

bool refused(int grid, const void* group_films, uint32_t film_pixels, const void* px, uint32_t n_own, uint32_t groups, const void* packed) {
    return groups == 0 || groups > PT_LIGHT_GROUPS_MAX || n_own == 0 || n_own > film_pixels || grid <= 0 || !group_films || !px || !packed;
}

}  // namespace

namespace ptk {

hipError_t launch_light_groups_pack(int grid, hipStream_t stream, const float* group_films, uint32_t film_pixels, const uint32_t* px, uint32_t n_own, uint32_t groups,
                                    float* packed) {
    if (refused(grid, group_films, film_pixels, px, n_own, groups, packed)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_light_groups_pack, dim3(grid), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(group_films), film_pixels, px, n_own, groups,
                       reinterpret_cast<float4*>(packed));
    return hipGetLastError();
}

hipError_t launch_light_groups_unpack(int grid, hipStream_t stream, const float* packed, const uint32_t* px, uint32_t n_own, uint32_t groups, float* group_films,
                                      uint32_t film_pixels) {
    if (refused(grid, group_films, film_pixels, px, n_own, groups, packed)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_light_groups_unpack, dim3(grid), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(packed), px, n_own, groups,
                       reinterpret_cast<float4*>(group_films), film_pixels);
    return hipGetLastError();
}

}  // namespace ptk
