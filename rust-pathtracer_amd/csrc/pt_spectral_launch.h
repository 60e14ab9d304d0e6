// pt_spectral_launch.h — launcher of the spectral accumulate kernel (pt_spectral.hip) that render_impl (pt_engine.hip) calls behind k_accumulate.
#ifndef PT_SPECTRAL_LAUNCH_H
#define PT_SPECTRAL_LAUNCH_H
#include <hip/hip_runtime.h>

#include "pt_stages.h"

namespace ptk {

// The pass `rp` describes (chunk_pixels items of the device list `pixels`, pass_samples samples each, in `energy`) added to spectral: bins planes of
// plane_pixels floats.  nl = 1 | 4 wavelengths per path; grid workgroups of 256 lanes on `stream`.  1 <= bins <= PT_SPECTRAL_MAX_BINS.
hipError_t launch_accumulate_spectral(int nl, int grid, hipStream_t stream, const ptd::RenderParams& rp, const uint32_t* pixels, const float* energy,
                                      float* spectral, uint32_t bins, uint32_t plane_pixels);

}  // namespace ptk
#endif
