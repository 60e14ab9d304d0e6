// pt_path_passes_launch.h — launchers of a path-pass render's two kernels (include/pt_light_groups.h): the vertex and light-sample forms
// that route energy to the planes of the path classes (pt_kern_passes.hip).  Everything behind them is a group render's (pt_light_groups_launch.h).
#ifndef PT_PATH_PASSES_LAUNCH_H
#define PT_PATH_PASSES_LAUNCH_H
#include "pt_launch.h"
#include "pt_path_pass_rules.h"

namespace ptk {

// launch_shade_groups and launch_shadow_groups without a table: `energy` holds pp_planes() planes of rp.energy_stride (energy_stride) slots, the last of them
// the state words
void launch_shade_passes(const LaunchCfg& c, const SceneArgs& sc, const ptd::RenderParams& rp, uint32_t bounce, const uint32_t* pixels, ptd::Queue paths_in, ptd::Queue hits,
                         ptd::Queue paths_out, ptd::Queue shadow, float* energy, uint32_t seg_cap, const uint32_t* count_in, uint32_t* count_out, uint32_t* shadow_count,
                         unsigned long long* block_stats);
void launch_shadow_passes(const LaunchCfg& c, const SceneArgs& sc, uint32_t light_samples, ptd::Queue shadow, float* energy, uint32_t energy_stride, uint32_t seg_cap,
                          const uint32_t* count_in);
hipError_t allow_lds_passes(uint32_t shade_bytes, uint32_t shadow_bytes);

}  // namespace ptk
#endif
