// pt_denoise_launch.h — launchers of the guide pass (pt_denoise.hip) that pt_render_guides (pt_engine.hip, where pt_scene lives) calls between the
// closest-hit probe's launches.  Every pointer is device memory of the current device; the launches go to the null stream.
#ifndef PT_DENOISE_LAUNCH_H
#define PT_DENOISE_LAUNCH_H
#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_denoise_rules.h"
#include "pt_stages.h"

namespace ptk {

// camera sample `sample` of every pixel 0 .. n_pixels-1 of the render `rp` describes (rp.chunk_pixels 1, as pt_camera_samples sets it): origins and directions, 3 floats each
void launch_guide_rays(const ptd::RenderParams& rp, uint32_t n_pixels, uint32_t sample, float* origins, float* directions);
// sums[p] += hits[p] (valid hits only); `first`: the sums start from zero
void launch_guide_fold(uint32_t n_pixels, const pt_hit* hits, ptd::DnGuideSum* sums, bool first);
// guides[p] = (N / samples, hits ? Z / hits : 0)
void launch_guide_finish(uint32_t n_pixels, const ptd::DnGuideSum* sums, uint32_t samples, float* guides_xyzw);

// The albedo guide.  layer_off: the blob word offsets of the `rows` texture layers of the scene's Lambertian materials; table: rows x 16 float4, the layers'
// curve values at the basis wavelengths; material_row[m]: the first row of material m's layers.  albedo_sums: n_pixels float4.
void albedo_basis(float wavelength_lo, float wavelength_hi, ptd::DnAlbedoBasis* basis);   // (host)
void launch_albedo_tables(const uint32_t* blob, const float* tex, const ptd::DnAlbedoBasis& basis, uint32_t rows, const uint32_t* layer_off, float* table);
// launch_guide_fold plus albedo_sums[p] += the hit's albedo
void launch_guide_fold_albedo(uint32_t n_pixels, const pt_hit* hits, ptd::DnGuideSum* sums, float* albedo_sums, bool first, const uint32_t* blob, const float* tex,
                              uint32_t material_count, const uint32_t* material_row, const float* table, const ptd::DnAlbedoBasis& basis);
// launch_guide_finish plus albedo[p] = albedo_sums[p] / samples (W = 0)
void launch_guide_finish_albedo(uint32_t n_pixels, const ptd::DnGuideSum* sums, const float* albedo_sums, uint32_t samples, float* guides_xyzw, float* albedo_xyzw);

}  // namespace ptk
#endif
