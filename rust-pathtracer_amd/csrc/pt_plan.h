// pt_plan.h — host-side planning shared by the HIP engine: film tiles -> pixel list of a shard,
// sample passes aligned to the reference's 10-sample phases, the choice of kernel forms for a scene and a render, thin-lens camera frame.
#ifndef PT_PLAN_H
#define PT_PLAN_H
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pt_adaptive.h"
#include "../../include/pt_api.h"
#include "../../include/pt_denoise.h"
#include "../../include/pt_light_groups.h"
#include "../../include/pt_light_groups_denoise.h"
#include "../../include/pt_resident.h"
#include "../../include/pt_spectral.h"
#include "pt_forms.h"
#include "pt_stages.h"

namespace pth {

// Pixels (linear id y * width + x) this call renders, tile by tile in the reference's tile order
// (TiledRenderer::generate_tiles, src/renderer/tiled.rs:190-277), row-major inside a tile; tiles are dealt
// round-robin to shards (tile t belongs to shard t % shard_count).
std::vector<uint32_t> shard_pixels(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h,
                                   uint32_t shard_index, uint32_t shard_count);

struct Pass { uint32_t pixel_begin, pixel_count, first_sample, sample_count; };
// Passes over (pixel chunk, sample range).  A pass never splits one of the reference's phases of 10 samples
// (tiled.rs:347-361) unless the requested range itself does, so the film sums keep the reference's order.
std::vector<Pass> plan_passes(uint32_t n_pixels, uint32_t first_sample, uint32_t sample_count, uint32_t capacity, uint32_t phase_samples = 10);

// Pass overlap: which of the pass loop's passes runs where, and behind what.  Consecutive passes run on two streams with two sets of pass buffers, so that one
// pass's launch tails and thin late bounces are filled with the next pass's early launches.  Pass p takes set and stream p % 2 (`lane`; 0 = the caller's
// stream), so pass p + 2 follows pass p in stream order and at most two passes are in flight.  Everything else is an event:
//   wait_fork         its first launch waits for the event recorded on the caller's stream when the pass loop began (the first pass of the second stream)
//   start_after       the pass behind whose bounce `signal_bounce` its first launch waits (-1 = none): two passes started together would run in lock step,
//                     their tails on top of each other
//   accumulate_after  the pass behind whose accumulate stage its own waits (-1 = none): the film sums keep the pass order
//   signal_bounce     the bounce behind whose launches it records the event the next pass starts after (-1 = none)
// join_pass: the pass behind whose accumulate stage the caller's stream waits before the loop returns (-1 = none: the last pass ran on it, behind every other).
struct PassStep { uint32_t lane; bool wait_fork; int32_t start_after, accumulate_after, signal_bounce; };
struct PassSchedule { std::vector<PassStep> steps; int32_t join_pass = -1; };
// bounces: the vertex launches of a pass; skew_bounce: the bounce g a pass signals behind (clamped to the last one), < 0 = the passes start together;
// overlap false, or fewer than two passes: every pass on lane 0, no event at all.
PassSchedule schedule_passes(uint32_t n_passes, uint32_t bounces, int32_t skew_bounce, bool overlap);
constexpr int32_t kPassSkewBounce = 0;   // the default g: measured best on C2 (profiles/pass_overlap.md)

// ---- Which kernel forms a scene and a render take (pt_forms.h): pure functions of plain inputs, for the engine and — exported by the host emulation, pinned by
// tests/golden/render_plans.tsv — for a machine without a device.
// What a scene decides once, when it is created: the tuning's edits of the blob (the PT_TUNE_* flags that are PT_FLAG_* bits, NO_MESH_SHORTCUTS, NO_CONVEX, the
// light-prepass limit) are applied to `blob` in place; lacks: the PT_SCENE_* bits of what the scene does not hold; lds_mode: PT_LDS_*, what the kernels stage.
struct ScenePlan { uint32_t lacks = 0; int lds_mode = 0; };
__attribute__((visibility("hidden"))) ScenePlan plan_scene(const pt_tuning& tn, std::vector<uint32_t>& blob);   // (hidden, as plan_render is: libptamd.so's exported names stay what they were)

// What a render asks of the plan beside the scene: the device's CUs, the normalised desc, the pixels of its list, the adaptive desc of an adaptive render,
// whether it is routed (light groups, path passes, path expressions: pt_kern_routed.hip), and the static LDS of the pooled traversal kernels (0: a product
// build, which has none; a measurement build passes ptk::pool_lds_bytes()).
struct RenderAsk {
    int num_cus = 0;
    pt_render_desc rd{};
    size_t n_pixels = 0;
    const pt_adaptive_desc* adaptive = nullptr;
    bool routed = false;
    uint32_t pool_lds_bytes = 0;
};
// What plan_render chooses for a render: the queues' size, the kernel forms and their launch configuration.
struct RenderPlan {
    uint32_t capacity = 0;   // path slots per pass
    int grid = 0;            // queue segments = workgroups per launch
    bool hero = false;       // four wavelengths per path
    uint32_t park_block = 0, park_block_extend = 0;   // the parked kernels' workgroups, big form or not (the scratch is sized by the first)
    int trav_form = 0, shade_form = 0;   // PT_FORM_*, PT_SHADE_*
    bool park_dynamic = false, park_big = false;
    uint32_t live_list = 0, camera_record = 0;   // RenderParams' fields of these names
    uint32_t path_fields = 0, item_fields = 0;
    // ptk::LaunchCfg's fields of these names (launch_*: its park_block and park_block_extend, 0 unless park_big)
    uint32_t lds_bytes = 0;
    int dyn_grid = 0;
    uint32_t walk_policy = 0;
    int launch_park_block = 0, launch_park_block_extend = 0;
    uint32_t park_blob_bytes = 0;
    bool certs = false, mesh_lights = false, fuse = false;
    bool overlap = false;    // the pass loop plans two passes or more somewhere, and the tuning lets them overlap: the render wants the second set of pass buffers
};
// The choices of a render, from the scene's blob (as plan_scene left it), its tuning and plan_scene's answer: false with the reason in *error for a
// pt_tuning::blocks_per_cu out of range.
__attribute__((visibility("hidden"))) bool plan_render(const std::vector<uint32_t>& blob, const pt_tuning& tn, const ScenePlan& scene, const RenderAsk& ask, RenderPlan* plan, std::string* error);

// ProjectiveCamera::new + with_aspect_ratio (src/camera/projective_camera.rs:27-95, 121-133)
ptd::CameraParams camera_params(const pt_camera& c, float aspect_ratio);

bool normalize_render_desc(const pt_render_desc& in, uint32_t camera_count, pt_render_desc* out, std::string* error);
// pt_render_adaptive's arguments (include/pt_adaptive.h), for the engine and the host emulation alike: PT_OK with the normalised render desc and
// adaptive desc (step 0 -> spp), or PT_ERR_INVALID_ARGUMENT / PT_ERR_UNSUPPORTED with the reason in *error.
pt_status normalize_adaptive_desc(const pt_render_desc& in, const pt_adaptive_desc& adaptive, bool has_sample_counts, uint32_t camera_count,
                                  pt_render_desc* out, pt_adaptive_desc* adaptive_out, std::string* error);

// pt_denoise_film's and pt_render_guides' arguments (include/pt_denoise.h), for the engine and the host emulation alike.  normalize_denoise_desc: PT_OK
// with the defaults filled in (iterations 0 -> 5, sigmas 0 -> 4 and 1, normal_power_log2 0 -> 7), or PT_ERR_INVALID_ARGUMENT with the reason in *error.
// check_denoise_inputs: every sample count at least 2 (the variance of a mean needs two samples), every guide value finite.
pt_status normalize_denoise_desc(const pt_denoise_desc* in, const void* film, const void* sample_counts, const void* stats, const void* guides, const void* out_film,
                                 pt_denoise_desc* out, std::string* error);
pt_status check_denoise_inputs(const pt_denoise_desc& d, const uint32_t* sample_counts, const float* guides, std::string* error);
pt_status check_guides_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const void* guides, std::string* error);
// pt_denoise_film_albedo's albedo plane (every channel finite and >= 0) and pt_albedo_basis' arguments
pt_status check_denoise_albedo(const pt_denoise_desc& d, const float* albedo, std::string* error);
pt_status check_albedo_basis_args(const pt_render_desc* rd, const void* lambda, const void* xyz, std::string* error);
// pt_render_guides_chain's arguments: the chain desc first (its refusals need no scene), then check_guides_args; *out = the desc with its default filled in
pt_status check_guides_chain_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                  const void* guides, pt_guide_chain_desc* out, std::string* error);
// The ID mattes' arguments (include/pt_denoise.h), for the engine and the host emulation alike; every refusal is PT_ERR_INVALID_ARGUMENT and names its argument.
// check_matte_args: the matte desc first (its refusals need no scene), then the scene and the render desc as check_guides_args judges them.
// check_matte_selections: set_count <= 16, offsets from 0 and never falling, at most 1024 keys.  check_matte_extract_args: the planes' size and ranks, then that.
pt_status check_matte_args(const void* scene, const pt_render_desc* rd, const pt_matte_desc* matte, uint32_t camera_count, std::string* error);
pt_status check_matte_selections(uint32_t set_count, const uint32_t* offsets, const uint32_t* selected, const void* out, std::string* error);
pt_status check_matte_extract_args(uint32_t width, uint32_t height, uint32_t ranks, const void* keys, const void* coverage, uint32_t set_count, const uint32_t* offsets,
                                   const uint32_t* selected, const void* out, std::string* error);
// What the extract kernel reads, in one array: 17 offsets (those behind set_count repeat the last) and behind them every selection sorted ascending without
// duplicates.  The arguments have passed check_matte_selections.
void matte_selection_words(uint32_t set_count, const uint32_t* offsets, const uint32_t* selected, std::vector<uint32_t>* words);

// pt_render_spectral's arguments (include/pt_spectral.h), for the engine and the host emulation alike, checked before the engine looks for a device:
// bins in 1..PT_SPECTRAL_MAX_BINS, reserved words 0, no null pointer; each refusal is PT_ERR_INVALID_ARGUMENT with its own message.  medium_aware
// is allowed (one wavelength per path, nothing about it differs), and everything else about the render desc is normalize_render_desc's to judge.
pt_status check_spectral_desc(const pt_spectral_desc* sd, std::string* error);
pt_status check_spectral_args(const void* scene, const pt_render_desc* rd, const pt_spectral_desc* sd, const void* film, const void* spectral, std::string* error);
// pt_spectral_bin_centres: centres_nm[b] = lo + ((float)b + 0.5f) * ((hi - lo) / (float)bins)
pt_status spectral_bin_centres(const pt_render_desc* rd, const pt_spectral_desc* sd, float* centres_nm, std::string* error);
// pt_render_adaptive_spectral's arguments: no null pointer (sample_counts included; stats may be null), check_spectral_desc's conditions, then
// normalize_adaptive_desc's, each with its own message; *rd_out and *ad_out as normalize_adaptive_desc leaves them.  The scene is only compared with null:
// camera_count is what the caller read from it.
pt_status check_adaptive_spectral_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_spectral_desc* sd, uint32_t camera_count,
                                       const void* film, const void* sample_counts, const void* spectral, pt_render_desc* rd_out, pt_adaptive_desc* ad_out,
                                       std::string* error);
// pt_render_spectral_multi's arguments: check_spectral_args' conditions, then no shard in the desc (the call deals the tiles itself) and
// normalize_render_desc's conditions, each with its own message; *rd_out as normalize_render_desc leaves it.  camera_count is what the caller read from the
// scene.  pt_render_adaptive_spectral_multi takes check_adaptive_spectral_args as it is: that refuses a shard too (normalize_adaptive_desc).
pt_status check_spectral_multi_args(const void* scene, const pt_render_desc* rd, const pt_spectral_desc* sd, uint32_t camera_count, const void* film, const void* spectral,
                                    pt_render_desc* rd_out, std::string* error);
// pt_denoise_spectral's arguments: bins in 1..PT_SPECTRAL_MAX_BINS and the two spectral pointers, then normalize_denoise_desc and check_denoise_inputs
pt_status check_denoise_spectral_args(const pt_denoise_desc* in, uint32_t bins, const void* film, const uint32_t* sample_counts, const void* stats, const float* guides,
                                      const void* spectral, const void* out_film, const void* out_spectral, pt_denoise_desc* out, std::string* error);
// pt_render_guides_bin_albedo's arguments: bins in 1..PT_SPECTRAL_MAX_BINS and the bin_albedo pointer, then check_guides_chain_args (chain null: the first
// hit, check_guides_args alone; *chain_out then has max_chain 0)
pt_status check_guides_bin_albedo_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                       uint32_t bins, const void* guides, const void* bin_albedo, pt_guide_chain_desc* chain_out, std::string* error);
// pt_denoise_spectral_albedo's arguments: check_denoise_spectral_args, then check_denoise_albedo on albedo (if given) and every bin_albedo value (if given)
// finite and >= 0
pt_status check_denoise_spectral_albedo_args(const pt_denoise_desc* in, uint32_t bins, const void* film, const uint32_t* sample_counts, const void* stats,
                                             const float* guides, const float* albedo, const void* spectral, const float* bin_albedo, const void* out_film,
                                             const void* out_spectral, pt_denoise_desc* out, std::string* error);
// A response matrix as pt_spectral_project and pt_spectral_project_resident take it: the matrix pointer, K in 1..PT_SPECTRAL_MAX_RESPONSES, bins in
// 1..PT_SPECTRAL_MAX_BINS, every entry finite; each refusal with its own message
pt_status check_spectral_matrix(uint32_t K, uint32_t bins, const float* matrix, std::string* error);
// pt_spectral_project's arguments: no null pointer, check_spectral_matrix, width and height positive and width x height within 31 bits
pt_status check_spectral_project_args(uint32_t width, uint32_t height, uint32_t bins, uint32_t K, const float* matrix, const void* spectral, const void* out,
                                      std::string* error);
// pt_spectral_response_matrix's arguments: no null pointer (curves / curve_data may be null when their counts are 0), check_spectral_desc, K and subsamples in
// range, the bounds in order, every response a curve index or a PT_RESPONSE_CIE_* constant, the filter a curve index or PT_SPECTRAL_NO_FILTER
pt_status check_response_matrix_args(const pt_render_desc* rd, const pt_spectral_desc* sd, const void* curves, uint32_t curve_count, const void* curve_data,
                                     uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, const void* matrix,
                                     std::string* error);

// ---- include/pt_resident.h.  `now`: what the scene holds resident (pt_resident_info's answer), so that the engine and the emulation refuse the same calls
// with the same words; every check runs before a device is looked for.
// the two halves of check_denoise_inputs, and the per-bin albedo's value check of check_denoise_spectral_albedo_args
pt_status check_denoise_counts(size_t n_pixels, const uint32_t* sample_counts, std::string* error);
pt_status check_denoise_guides(size_t n_pixels, const float* guides, std::string* error);
pt_status check_denoise_bin_albedo(size_t n_values, const float* bin_albedo, std::string* error);
pt_status check_resident_info_args(const void* scene, const void* info, std::string* error);
// pt_resident_guides: the flags known and BIN_ALBEDO only with ALBEDO; a resident film, of desc's size; BIN_ALBEDO only with resident bins; then
// check_guides_args, or check_guides_chain_args where a chain is given (*chain_out: normalised, max_chain 0 without one)
pt_status check_resident_guides_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                     uint32_t flags, const struct pt_resident_info& now, pt_guide_chain_desc* chain_out, std::string* error);
// pt_resident_load: something given; the size positive and within 31 bits; film, counts and stats together; bins in 1..64 with spectral or bin_albedo; the
// size (and bins) those of the parts that stay resident; the values as the host-array denoise entries want them
pt_status check_resident_load_args(const void* scene, uint32_t width, uint32_t height, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats,
                                   const float* spectral, const float* guides, const float* albedo, const float* bin_albedo, const struct pt_resident_info& now,
                                   std::string* error);
// pt_denoise_resident: the desc's flags and reserved words, its filter as normalize_denoise_desc wants it (*out: normalised, with the resident size), a
// resident film and resident guides, the size 0 or the resident one, out_spectral only with resident bins
pt_status check_resident_denoise_args(const void* scene, const pt_resident_denoise_desc* desc, const void* out_spectral, const struct pt_resident_info& now,
                                      pt_denoise_desc* out, std::string* error);
// pt_spectral_project_resident_denoised: pt_spectral_project_resident's checks, over the resident denoised bins
pt_status check_resident_project_args(const void* scene, uint32_t K, const float* matrix, const void* out, const struct pt_resident_info& now, std::string* error);
// What a scene remembers of its last adaptive node render (pt_render_adaptive_multi, pt_render_adaptive_spectral_multi over more than one device) while the
// pieces lie where that render left them: the size, the bins (0 without a spectral film) and whether the statistics were gathered.  Every render entry
// forgets it when it starts.
struct NodeRender {
    bool valid = false, stats = false;
    uint32_t width = 0, height = 0, bins = 0;
};
// pt_resident_assemble: the scene; the flags known; a node render to assemble; one made with stats — each refusal with its own message
pt_status check_resident_assemble(const void* scene, uint32_t flags, const NodeRender& node, std::string* error);
// pt_resident_read: a pointer that is given names a part that is resident (film_xyzw, sample_counts and stats: FILM; spectral: BINS)
pt_status check_resident_read_args(const void* scene, const void* film, const void* sample_counts, const void* stats, const void* spectral, const struct pt_resident_info& now,
                                   std::string* error);

// ---- include/pt_light_groups.h, for the engine and the host emulation alike; every check runs before a device is looked for.
// pt_render_light_groups: no null pointer (group_films may be null); group_count in 1..PT_LIGHT_GROUPS_MAX, reserved words 0, instance_count the scene's
// (`scene_instances`), every group id and the environment's below group_count: PT_ERR_INVALID_ARGUMENT.  hero_wavelengths 4, medium_aware, a shard
// (shard_count > 1) and a partial sample range: PT_ERR_UNSUPPORTED.  Everything else about the render desc is normalize_render_desc's to judge.
pt_status check_light_groups_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, const void* film,
                                  std::string* error);
// the matrices of a mix: the pointer, group_count in 1..PT_LIGHT_GROUPS_MAX, every entry finite
pt_status check_light_groups_matrices(uint32_t group_count, const float* matrices, std::string* error);
// pt_light_groups_mix: no null pointer, check_light_groups_matrices, width and height positive and width x height within 31 bits
pt_status check_light_groups_mix_args(uint32_t width, uint32_t height, uint32_t group_count, const void* group_films, const float* matrices, const void* out,
                                      std::string* error);

// pt_render_path_passes (include/pt_light_groups.h): no null pointer (pass_films may be null), reserved words 0: PT_ERR_INVALID_ARGUMENT; hero_wavelengths 4,
// medium_aware, a shard (shard_count > 1) and a partial sample range: PT_ERR_UNSUPPORTED, as check_light_groups_args refuses them
pt_status check_path_passes_args(const void* scene, const pt_render_desc* rd, const pt_path_passes_desc* pd, const void* film, std::string* error);
// pt_render_path_exprs (include/pt_light_groups.h, "Path expressions"): what check_path_passes_args refuses of a render desc; a malformed program — outputs
// outside 1..8, states outside 1..64, a start or successor not below states, a bit outside the successors and the masks of its outputs — and a group table that
// is not the scene's (null with n_instances 0, or one id below 8 per instance): PT_ERR_INVALID_ARGUMENT
pt_status check_path_exprs_args(const void* scene, const pt_render_desc* rd, const pt_path_expr_program* program, const uint8_t* instance_group, uint32_t n_instances,
                                uint32_t scene_instances, const void* film, std::string* error);
// pt_render_adaptive_path_exprs (include/pt_light_groups_denoise.h): the adaptive desc too, then check_path_exprs_args and normalize_adaptive_desc
pt_status check_adaptive_path_exprs_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_path_expr_program* program,
                                         const uint8_t* instance_group, uint32_t n_instances, uint32_t scene_instances, uint32_t camera_count, const void* film,
                                         const void* sample_counts, pt_render_desc* rd_out, pt_adaptive_desc* ad_out, std::string* error);
// pt_render_adaptive_path_passes (include/pt_light_groups_denoise.h): the adaptive desc too, then check_path_passes_args and normalize_adaptive_desc
pt_status check_adaptive_path_passes_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_path_passes_desc* pd, uint32_t camera_count,
                                          const void* film, const void* sample_counts, pt_render_desc* rd_out, pt_adaptive_desc* ad_out, std::string* error);

// ---- include/pt_light_groups_multi.h, for the engine and the host emulation alike; every check runs before a device is looked for.
// pt_render_light_groups_multi: everything check_light_groups_args refuses, with its words, except that a shard in the desc (shard_count != 0) is the node
// entry's own PT_ERR_INVALID_ARGUMENT ("... deals the tiles itself: shard_count must be 0"); then normalize_render_desc's conditions; *rd_out as that leaves it.
pt_status check_light_groups_multi_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, uint32_t camera_count,
                                        const void* film, pt_render_desc* rd_out, std::string* error);
// pt_render_adaptive_light_groups_multi: check_adaptive_light_groups_args with the same exchange of the shard refusal
pt_status check_adaptive_light_groups_multi_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_light_groups_desc* gd,
                                                 uint32_t scene_instances, uint32_t camera_count, const void* film, const void* sample_counts, pt_render_desc* rd_out,
                                                 pt_adaptive_desc* ad_out, std::string* error);

// ---- include/pt_light_groups_denoise.h, for the engine and the host emulation alike; every check runs before a device is looked for.
// pt_render_adaptive_light_groups: no null pointer (stats and group_films may be null), then everything check_light_groups_args refuses and everything
// normalize_adaptive_desc refuses, each with its own message; *rd_out and *ad_out as normalize_adaptive_desc leaves them.
pt_status check_adaptive_light_groups_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_light_groups_desc* gd, uint32_t scene_instances,
                                           uint32_t camera_count, const void* film, const void* sample_counts, pt_render_desc* rd_out, pt_adaptive_desc* ad_out,
                                           std::string* error);
// pt_denoise_light_groups: group_count in 1..PT_LIGHT_GROUPS_MAX and the two group-film pointers, then pt_denoise_spectral_albedo's rules (normalize_denoise_desc,
// check_denoise_inputs, check_denoise_albedo where an albedo is given)
pt_status check_denoise_light_groups_args(const pt_denoise_desc* in, uint32_t group_count, const void* film, const uint32_t* sample_counts, const void* stats,
                                          const float* guides, const float* albedo, const void* group_films, const void* out_film, const void* out_group_films,
                                          pt_denoise_desc* out, std::string* error);
// What a scene remembers of its group films for the resident entries: the last group render's size and count, whether that render was the adaptive one whose
// film is still the resident one (`paired`), and what pt_denoise_light_groups_resident left (`denoised`)
struct GroupsResident { bool valid = false, paired = false, denoised = false; uint32_t width = 0, height = 0, group_count = 0; };
// pt_denoise_light_groups_resident: the scene and the desc, flags 0, reserved words 0, the filter as normalize_denoise_desc wants it (*out: normalised, with the
// resident size), a resident film and guides, group films paired with that film, the size 0 or the resident one
pt_status check_resident_denoise_light_groups_args(const void* scene, const pt_resident_denoise_desc* desc, const struct pt_resident_info& now, const GroupsResident& groups,
                                                   pt_denoise_desc* out, std::string* error);

}  // namespace pth
#endif
