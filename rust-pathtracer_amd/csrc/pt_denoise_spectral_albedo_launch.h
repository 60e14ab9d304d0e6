// pt_denoise_spectral_albedo_launch.h — launchers of the per-bin albedo guide's kernels (pt_denoise_spectral_albedo.hip).
// Every pointer is device memory of the current device; the launches go to the null stream.  Planes are bin-major: `bins` planes of n_pixels floats.
#ifndef PT_DENOISE_SPECTRAL_ALBEDO_LAUNCH_H
#define PT_DENOISE_SPECTRAL_ALBEDO_LAUNCH_H
#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_bin_albedo_device.h"

namespace ptk {

// table: rows x bins float4, the curve values of the layers `layer_off` names (launch_albedo_tables' rows) at the bins' centres lo + ((float)b + 0.5f) * bin_width
void launch_bin_albedo_tables(const uint32_t* blob, const float* tex, float wavelength_lo, float bin_width, uint32_t bins, uint32_t rows, const uint32_t* layer_off, float* table);
// fold.sums[b * fold.plane + p] += the per-bin albedo of hits[p], p < n_pixels <= fold.plane (the sums start zeroed)
void launch_guide_fold_bins(uint32_t n_pixels, const pt_hit* hits, const BinAlbedoFold& fold, const uint32_t* blob, const float* tex, uint32_t material_count);
// bin_albedo = sums / samples, over bins x n_pixels values
void launch_bin_albedo_finish(uint32_t n_pixels, uint32_t bins, const float* sums, uint32_t samples, float* bin_albedo);

}  // namespace ptk
#endif
