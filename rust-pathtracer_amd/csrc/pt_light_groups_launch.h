// pt_light_groups_launch.h — launchers of what lies behind a routed render's vertex and light-sample forms (pt_routed_launch.h), for light groups and path passes
// alike (include/pt_light_groups.h, DESIGN.md sections 15 and 17): the per-group accumulate kernel, the adaptive finish and the mix (pt_light_groups.hip).
#ifndef PT_LIGHT_GROUPS_LAUNCH_H
#define PT_LIGHT_GROUPS_LAUNCH_H
#include "pt_launch.h"
#include "pt_light_group_rules.h"

namespace ptk {

// group g's film (group_films + g * 4 * film_pixels floats) += the pass's samples of plane 2 + g, every pixel by lg_accumulate_pixel
hipError_t launch_accumulate_groups(hipStream_t stream, const ptd::RenderParams& rp, const uint32_t* pixels, const float* energy, float* group_films, uint32_t group_count,
                                    size_t film_pixels);
// the finish of an adaptive group render: every pixel of every group film divided by its own count (lg_adaptive_finish_pixel)
hipError_t launch_adaptive_finish_groups(hipStream_t stream, uint32_t n_pixels, const uint32_t* counts, float* group_films, uint32_t group_count);
// out (n_pixels float4) = the mix of group_count films of n_pixels float4 by `matrices` (group_count x 9 floats, device memory), every pixel by lg_mix_pixel
hipError_t launch_light_groups_mix(hipStream_t stream, uint32_t n_pixels, uint32_t group_count, const float* group_films, const float* matrices, float* out);

}  // namespace ptk
#endif
