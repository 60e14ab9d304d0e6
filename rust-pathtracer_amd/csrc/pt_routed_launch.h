// pt_routed_launch.h — launchers of a routed render's two kernels (pt_kern_routed.hip; pt_routed_rules.h): the vertex and light-sample forms of a light-group
// render (GroupRouter), of a path-pass render (section 17, PassRouter) and of a path-expression render (section 17, ExprRouter).  Everything behind them is pt_light_groups_launch.h's.
#ifndef PT_ROUTED_LAUNCH_H
#define PT_ROUTED_LAUNCH_H
#include "pt_launch.h"
#include "pt_path_expr_rules.h"

namespace ptk {

// launch_shade's FULL form, one wavelength, unfused, and launch_shadow's general form, each with a router (instantiated for GroupRouter, PassRouter and ExprRouter).
// `energy`: the router's planes of rp.energy_stride (energy_stride) slots behind the total and the wavelength samples — lg_planes(G) for groups (instance_group:
// device memory, one byte per instance), pp_planes() for passes, the last of them the state words the PassRouter points at, px_planes(K) for K expressions likewise (table and
// instance_group: device memory).
template <typename Router>
void launch_shade_routed(const LaunchCfg& c, const SceneArgs& sc, const ptd::RenderParams& rp, uint32_t bounce, const uint32_t* pixels, ptd::Queue paths_in, ptd::Queue hits,
                         ptd::Queue paths_out, ptd::Queue shadow, float* energy, uint32_t seg_cap, const uint32_t* count_in, uint32_t* count_out, uint32_t* shadow_count,
                         unsigned long long* block_stats, const Router& router);
template <typename Router>
void launch_shadow_routed(const LaunchCfg& c, const SceneArgs& sc, uint32_t light_samples, ptd::Queue shadow, float* energy, uint32_t energy_stride, uint32_t seg_cap,
                          const uint32_t* count_in, const Router& router);
hipError_t allow_lds_routed(uint32_t shade_bytes, uint32_t shadow_bytes);

}  // namespace ptk
#endif
