// pt_spectral_shard_launch.h — launchers of the pack kernel (pt_spectral_shard.hip) that the node entries of pt_engine.hip run behind a device's render, and of
// the unpack kernel that pt_resident_assemble runs over every shard.
#ifndef PT_SPECTRAL_SHARD_LAUNCH_H
#define PT_SPECTRAL_SHARD_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {

// packed (bins planes of n_own floats) = the n_own pixels px (a device list) of planes (bins planes of plane_pixels floats), by spectral_shard_pack_item.
// 1 <= bins <= PT_SPECTRAL_MAX_BINS, n_own >= 1, every px[i] < plane_pixels (the callers' lists are pth::shard_pixels'); `grid` workgroups of 256 lanes on
// `stream`.  The kernel moves n_own * (4 + 8 * bins) bytes.
hipError_t launch_spectral_pack(int grid, hipStream_t stream, const float* planes, uint32_t plane_pixels, const uint32_t* px, uint32_t n_own, uint32_t bins, float* packed);
// The inverse: the n_own pixels px of planes (bins planes of plane_pixels floats) = packed (bins planes of n_own floats), by spectral_shard_unpack_item; the
// other floats of planes are not written.  The same limits, refused the same way; px holds no pixel twice, so no two lanes write the same float.  `grid`:
// spectral_pack_grid's.
hipError_t launch_spectral_unpack(int grid, hipStream_t stream, const float* packed, const uint32_t* px, uint32_t n_own, uint32_t bins, float* planes, uint32_t plane_pixels);
// One workgroup per 256 items, at most 8 per compute unit (the grid-stride loop takes the rest)
inline int spectral_pack_grid(int compute_units, uint32_t n_own) {
    const uint32_t need = (n_own + 255u) / 256u, cap = (uint32_t)(compute_units > 0 ? compute_units : 1) * 8u;
    return (int)(need < cap ? need : cap);
}

}  // namespace ptk
#endif
