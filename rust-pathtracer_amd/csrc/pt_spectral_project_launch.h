// pt_spectral_project_launch.h — launcher of the development kernel (pt_spectral_project.hip) for the host-array entry there and the resident entry of
// pt_engine.hip.
#ifndef PT_SPECTRAL_PROJECT_LAUNCH_H
#define PT_SPECTRAL_PROJECT_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {

// out (K planes of n_pixels floats) = matrix (K x bins, row-major, device memory) times spectral (bins planes of n_pixels floats), every pixel by
// spectral_project_pixel: at most 8 responses per pass over the planes, so K <= 8 is one launch and K <= 16 two.  1 <= K <= PT_SPECTRAL_MAX_RESPONSES,
// 1 <= bins <= PT_SPECTRAL_MAX_BINS, 1 <= n_pixels <= 2^31 - 1 (the callers' argument checks); `grid` workgroups of 256 lanes on `stream`.
hipError_t launch_spectral_project(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t bins, uint32_t K, const float* matrix, const float* spectral, float* out);
// The grid both entries launch: one workgroup per 256 pixels, at most 8 per compute unit (the grid-stride loop takes the rest)
inline int spectral_project_grid(int compute_units, uint32_t n_pixels) {
    const uint32_t need = (n_pixels + 255u) / 256u, cap = (uint32_t)(compute_units > 0 ? compute_units : 1) * 8u;
    return (int)(need < cap ? need : cap);
}

}  // namespace ptk
#endif
