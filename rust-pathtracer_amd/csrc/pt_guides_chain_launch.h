// pt_guides_chain_launch.h — launchers of the specular-chain guide pass (pt_guides_chain.hip) that pt_render_guides_chain (pt_engine.hip, where pt_scene
// lives) calls around the closest-hit probe's launches.  Every pointer is device memory of the current device; the launches go to the null stream.
#ifndef PT_GUIDES_CHAIN_LAUNCH_H
#define PT_GUIDES_CHAIN_LAUNCH_H
#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_bin_albedo_device.h"
#include "pt_denoise_rules.h"
#include "pt_stages.h"

namespace ptk {

// A list of rays for the probe (origins and directions, 3 floats each) with what each ray carries along its chain: its pixel, its wavelength, the path
// length so far (one uint4 per ray: pixel, wavelength bits, length bits, 0).
struct ChainRays { float* o; float* d; uint4* state; };
// the albedo inputs of launch_guide_fold_albedo (pt_denoise_launch.h); albedo_sums null: the guides alone
// bin_fold (sums null: none; needs albedo_sums): the per-bin albedo's sums, folded at the same terminal vertex (pt_render_guides_bin_albedo)
struct ChainAlbedo { float* albedo_sums; const uint32_t* material_row; const float* table; ptd::DnAlbedoBasis basis; BinAlbedoFold bin_fold; };

// camera sample `sample` of every pixel 0 .. n_pixels-1 (launch_guide_rays' rays) as the chain's vertex-0 list: ray i is pixel i's, length 0
void launch_chain_rays(const ptd::RenderParams& rp, uint32_t n_pixels, uint32_t sample, const ChainRays& out);
// One vertex of the chain for the `n` rays of `in`, whose closest hits are `hits`: a ray that ends here (miss, terminal vertex) folds into its pixel's sums;
// one that goes on is appended to `out` at the position *count_out hands it (zero before the launch; the number of rays of `out` after it).
void launch_chain_step(uint32_t n, const pt_hit* hits, const ChainRays& in, const ChainRays& out, uint32_t* count_out, ptd::DnGuideSum* sums, const ChainAlbedo& albedo,
                       uint32_t vertex, uint32_t max_chain, float alpha_max, const uint32_t* blob, const float* tex, uint32_t material_count);

}  // namespace ptk
#endif
