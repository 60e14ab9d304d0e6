// pt_light_groups_launch.h — launchers of a light-group render's kernels (include/pt_light_groups.h): the vertex and light-sample forms that
// route energy to group planes (pt_kern_groups.hip), the per-group accumulate kernel and the mix (pt_light_groups.hip).
#ifndef PT_LIGHT_GROUPS_LAUNCH_H
#define PT_LIGHT_GROUPS_LAUNCH_H
#include "pt_launch.h"
#include "pt_light_group_rules.h"

namespace ptk {

// launch_shade's FULL form, one wavelength, unfused, and launch_shadow's general form, each with `groups` (instance_group: device memory, one byte per instance)
void launch_shade_groups(const LaunchCfg& c, const SceneArgs& sc, const ptd::RenderParams& rp, uint32_t bounce, const uint32_t* pixels, ptd::Queue paths_in, ptd::Queue hits,
                         ptd::Queue paths_out, ptd::Queue shadow, float* energy, uint32_t seg_cap, const uint32_t* count_in, uint32_t* count_out, uint32_t* shadow_count,
                         unsigned long long* block_stats, const ptd::LightGroupTable& groups);
void launch_shadow_groups(const LaunchCfg& c, const SceneArgs& sc, uint32_t light_samples, ptd::Queue shadow, float* energy, uint32_t energy_stride, uint32_t seg_cap,
                          const uint32_t* count_in, const ptd::LightGroupTable& groups);
hipError_t allow_lds_groups(uint32_t shade_bytes, uint32_t shadow_bytes);

// group g's film (group_films + g * 4 * film_pixels floats) += the pass's samples of plane 2 + g, every pixel by lg_accumulate_pixel
hipError_t launch_accumulate_groups(hipStream_t stream, const ptd::RenderParams& rp, const uint32_t* pixels, const float* energy, float* group_films, uint32_t group_count,
                                    size_t film_pixels);
// the finish of an adaptive group render: every pixel of every group film divided by its own count (lg_adaptive_finish_pixel)
hipError_t launch_adaptive_finish_groups(hipStream_t stream, uint32_t n_pixels, const uint32_t* counts, float* group_films, uint32_t group_count);
// out (n_pixels float4) = the mix of group_count films of n_pixels float4 by `matrices` (group_count x 9 floats, device memory), every pixel by lg_mix_pixel
hipError_t launch_light_groups_mix(hipStream_t stream, uint32_t n_pixels, uint32_t group_count, const float* group_films, const float* matrices, float* out);

}  // namespace ptk
#endif
