// pt_denoise_spectral_launch.h — launchers of the joint filter's kernels (pt_denoise_spectral.hip).  Every pointer is device memory of the current
// device; the launches go to the null stream.  The buffers are pt_denoise_launch.h's (launch_dn_prepare, launch_dn_tent) plus the bins: `bins` planes of
// width * height floats, 1 <= bins <= PT_SPECTRAL_MAX_BINS.
#ifndef PT_DENOISE_SPECTRAL_LAUNCH_H
#define PT_DENOISE_SPECTRAL_LAUNCH_H
#include <hip/hip_runtime.h>

#include "pt_denoise_rules.h"

namespace ptk {

// flags[p] |= DN_DEAD where a bin of pixel p is not finite (behind launch_dn_prepare)
void launch_dn_spectral_dead(uint32_t n_pixels, uint32_t bins, const float* spectral, uint8_t* flags);
// one a-trous pass of step `step`: color_out = c_{i+1}, v_{i+1} (k_dn_gather's, bit for bit) and spectral_out = s_{b,i+1} for every bin, each tap's weight
// computed once per pixel.  tent: launch_dn_tent's output for this pass.  The outputs must not alias the inputs.
void launch_dn_gather_spectral(const ptd::DnParams& P, int step, const float* color, const float* geo, const float* tent, const uint8_t* flags, const float* grad,
                               uint32_t bins, const float* spectral, float* color_out, float* spectral_out);

}  // namespace ptk
#endif
