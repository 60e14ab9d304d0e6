// pt_light_groups_shard_launch.h — launchers of the pack kernel (pt_light_groups_shard.hip) that the group node entries of pt_engine.hip run behind a device's
// render, and of the unpack kernel that pt_resident_assemble runs over every group shard.
#ifndef PT_LIGHT_GROUPS_SHARD_LAUNCH_H
#define PT_LIGHT_GROUPS_SHARD_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {

// packed (groups films of n_own float4) = the n_own pixels px (a device list) of group_films (groups films of film_pixels float4), by lg_shard_pack_item.
// 1 <= groups <= PT_LIGHT_GROUPS_MAX, 1 <= n_own <= film_pixels, every px[i] < film_pixels (the callers' lists are pth::shard_pixels'), both arrays 16-byte
// aligned; `grid` workgroups of 256 lanes on `stream`.  The kernel moves n_own * (4 + 32 * groups) bytes.
hipError_t launch_light_groups_pack(int grid, hipStream_t stream, const float* group_films, uint32_t film_pixels, const uint32_t* px, uint32_t n_own, uint32_t groups,
                                    float* packed);
// The inverse: the n_own pixels px of group_films = packed, by lg_shard_unpack_item; the other pixels of group_films are not written.  The same limits, refused
// the same way; px holds no pixel twice, so no two lanes write the same pixel.
hipError_t launch_light_groups_unpack(int grid, hipStream_t stream, const float* packed, const uint32_t* px, uint32_t n_own, uint32_t groups, float* group_films,
                                      uint32_t film_pixels);
// One workgroup per 256 items, at most 8 per compute unit (the grid-stride loop takes the rest)
inline int light_groups_pack_grid(int compute_units, uint32_t n_own) {
    const uint32_t need = (n_own + 255u) / 256u, cap = (uint32_t)(compute_units > 0 ? compute_units : 1) * 8u;
    return (int)(need < cap ? need : cap);
}

}  // namespace ptk
#endif
