// pt_shard_launch.h — launchers of the pack kernels (pt_shard.hip) that the spectral and the group node entries of pt_engine.hip run behind a device's render,
// and of the unpack kernels that pt_resident_assemble runs over every shard.
#ifndef PT_SHARD_LAUNCH_H
#define PT_SHARD_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {

// elem_floats is the element of pt_shard_rules.h: 1, floats (k_spectral_pack / k_spectral_unpack; planes <= PT_SPECTRAL_MAX_BINS), or 4, pixels of four
// floats (k_light_groups_pack / k_light_groups_unpack; planes <= PT_LIGHT_GROUPS_MAX, both arrays 16-byte aligned).  Anything else is refused.
//
// packed (`planes` planes of n_own elements) = the n_own pixels px (a device list) of full (`planes` planes of full_pixels elements), by shard_pack_item.
// planes >= 1, 1 <= n_own <= full_pixels, every px[i] < full_pixels (the callers' lists are pth::shard_pixels'); `grid` workgroups of 256 lanes on `stream`
// (shard_pack_grid's).  The kernel moves n_own * (4 + 8 * elem_floats * planes) bytes.
hipError_t launch_shard_pack(uint32_t elem_floats, int grid, hipStream_t stream, const float* full, uint32_t full_pixels, const uint32_t* px, uint32_t n_own, uint32_t planes,
                             float* packed);
// The inverse: the n_own pixels px of full = packed, by shard_unpack_item; the other elements of full are not written.  The same limits, refused the same
// way; px holds no pixel twice, so no two lanes write the same element.
hipError_t launch_shard_unpack(uint32_t elem_floats, int grid, hipStream_t stream, const float* packed, const uint32_t* px, uint32_t n_own, uint32_t planes, float* full,
                               uint32_t full_pixels);
// One workgroup per 256 items, at most 8 per compute unit (the grid-stride loop takes the rest)
inline int shard_pack_grid(int compute_units, uint32_t n_own) {
    const uint32_t need = (n_own + 255u) / 256u, cap = (uint32_t)(compute_units > 0 ? compute_units : 1) * 8u;
    return (int)(need < cap ? need : cap);
}

}  // namespace ptk
#endif
