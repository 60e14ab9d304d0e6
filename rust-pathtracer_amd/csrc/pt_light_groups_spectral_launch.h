// pt_light_groups_spectral_launch.h — launchers of the kernels of spectral light groups (pt_light_groups_spectral.hip; include/pt_light_groups_spectral.h,
// DESIGN.md section 15) for the host-array entry there and the render and resident entries of pt_engine.hip.
#ifndef PT_LIGHT_GROUPS_SPECTRAL_LAUNCH_H
#define PT_LIGHT_GROUPS_SPECTRAL_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_stages.h"

namespace ptk {

// group g's bins (group_spectral + g * bins * plane_pixels floats, bins planes of plane_pixels) += the pass's samples of plane 2 + g, every pixel by
// lg_spectral_fold_pixel.  1 <= group_count <= PT_LIGHT_GROUPS_MAX, 1 <= bins <= PT_SPECTRAL_MAX_BINS; every pixel id of `pixels` is below plane_pixels.
hipError_t launch_accumulate_group_bins(hipStream_t stream, const ptd::RenderParams& rp, const uint32_t* pixels, const float* energy, float* group_spectral,
                                        uint32_t group_count, uint32_t bins, uint32_t plane_pixels);
// out (K planes of n_pixels floats) = matrix (K x planes, row-major, device memory) times group_spectral (planes = G * bins planes of n_pixels floats), every
// pixel by spectral_project_pixel: at most 8 responses per pass over the planes.  1 <= K <= PT_SPECTRAL_MAX_RESPONSES, 1 <= planes <= 512,
// 1 <= n_pixels <= 2^31 - 1 (the callers' argument checks); `grid` workgroups of 256 lanes on `stream` (spectral_project_grid).
hipError_t launch_light_groups_relamp(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t planes, uint32_t K, const float* matrix, const float* group_spectral,
                                      float* out);

}  // namespace ptk
#endif
