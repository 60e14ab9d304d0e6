/* pt_light_groups_denoise.h — adaptive and denoised light groups: relight a filtered render.  The second half of the light-group surface; pt_light_groups.h keeps
 * the fixed-count render and the mix as they are.  Exported by libptamd.so (pt_); the rules are also compiled into the host emulation of the tests
 * (ptemu_render_adaptive_light_groups, ptemu_denoise_light_groups).  The definition is DESIGN.md section 15, "Adaptive and denoised group films"; in short:
 *
 *   The adaptive group render is pt_render_adaptive — film, counts, statistics, rounds and ray counters bit for bit: the stop decisions read the total film's
 *   statistics alone — that also leaves one film per group.  Group g's film at pixel p is pt_render_light_groups' group film at spp = sample_counts[p], bit for
 *   bit; with max_samples == spp the group films are pt_render_light_groups' bit for bit.
 *
 *   The joint filter over group films.  With G groups take the 3G planes P[3g + c] = channel c of group g's film and, where albedo_xyzw is given,
 *   A[3g + c] = albedo channel c (otherwise no per-bin albedo).  out_film_xyzw, out_variance and the X, Y, Z of out_group_films are bit for bit what
 *   pt_denoise_spectral_albedo(desc, 3G, film, counts, stats, guides, albedo_xyzw, P, A, ...) returns.  So: the taps and weights are pt_denoise_film(_albedo)'s,
 *   computed once per pixel and pass from the TOTAL film; every group channel is averaged as sb / sw in tap order; the divisor is max(albedo, 1e-3f), divided
 *   out before the passes and multiplied back after the last; a pixel is dead, and all its float4s are copied through, when the film calls it dead or any group
 *   channel is not finite before or after the division.  A live pixel's w is 0.  Demodulation is sound for groups: the first-hit albedo does not depend on which
 *   lamp lit the pixel.
 *
 * Layout of group films: pt_light_groups.h's, group_films[((g * height + y) * width + x) * 4 + c]. */
#ifndef PT_LIGHT_GROUPS_DENOISE_H
#define PT_LIGHT_GROUPS_DENOISE_H
#include "pt_adaptive.h"
#include "pt_denoise.h"
#include "pt_light_groups.h"
#include "pt_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

/* desc, adaptive, film_xyzw, sample_counts, stats (may be NULL): pt_render_adaptive's; groups, group_films (may be NULL): pt_render_light_groups'.  Refused is
 * what either of them refuses: hero_wavelengths 4, medium_aware, a shard, a partial sample range, a bad group table, a bad adaptive desc, each with its own
 * message.  On success the scene holds resident FILM as after pt_render_adaptive (pt_resident_info, pt_resident_guides follow) and the group films as after
 * pt_render_light_groups (pt_light_groups_resident, pt_light_groups_mix_resident), and remembers that the two came from one render: that pairing ends when
 * the resident film is ended or replaced (any render entry, pt_resident_load with a film, pt_resident_assemble) or another group render starts. */
pt_status pt_render_adaptive_light_groups(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, const pt_light_groups_desc* groups,
                                          float* film_xyzw, uint32_t* sample_counts, double* stats, float* group_films, pt_profile* profile);

/* The joint filter of host arrays.  The argument rules are pt_denoise_spectral_albedo's, plus 1 <= group_count <= PT_LIGHT_GROUPS_MAX.  albedo_xyzw and
 * out_variance may be NULL.  group_films, out_group_films: group_count * width * height * 4 f32; out_group_films may be group_films. */
pt_status pt_denoise_light_groups(const pt_denoise_desc* desc, uint32_t group_count, const float* film_xyzw, const uint32_t* sample_counts, const double* stats,
                                  const float* guides_xyzw, const float* albedo_xyzw, const float* group_films, float* out_film_xyzw, float* out_variance,
                                  float* out_group_films);

/* The filter over resident FILM, GUIDES (ALBEDO selects demodulation) and the group films paired with that film (pt_render_adaptive_light_groups).  desc->flags
 * must be 0.  The outputs are bit for bit pt_denoise_light_groups' for the arrays the render and guide entries returned.  Every out pointer may be NULL, and
 * nothing crosses the bus for a NULL one.  The sources are not written, so the call may be repeated with other parameters; the scratch and the denoised group
 * films are kept with the scene, so a repeated call allocates nothing.  The PT_RESIDENT_* parts and pt_denoise_resident's outputs are untouched.  The denoised
 * group films stay until the next group render of either kind, the next call of this entry, or the scene's end. */
pt_status pt_denoise_light_groups_resident(pt_scene* scene, const pt_resident_denoise_desc* desc, float* out_film_xyzw, float* out_variance, float* out_group_films);

/* What pt_denoise_light_groups_resident left on the scene's device: its size and group count, or three zeros when there is none. */
pt_status pt_light_groups_denoised_resident(pt_scene* scene, uint32_t* width, uint32_t* height, uint32_t* group_count);

/* pt_light_groups_mix over the resident denoised group films: the matrices go up (at most 72 floats), one film comes back. */
pt_status pt_light_groups_mix_resident_denoised(pt_scene* scene, const float* matrices, float* out_xyzw);

/* pt_render_path_passes (pt_light_groups.h) under pt_render_adaptive's stop rule: film, counts, statistics and rounds are pt_render_adaptive's bit for bit, and
 * pass c's film at pixel p is pt_render_path_passes' at spp = sample_counts[p].  On success the scene holds the resident FILM and the eight pass films as its
 * group films, paired as after pt_render_adaptive_light_groups: pt_denoise_light_groups_resident follows.  (The return type on a line of its own, as
 * there and for the same reason.) */
pt_status
pt_render_adaptive_path_passes(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, const pt_path_passes_desc* passes, float* film_xyzw,
                               uint32_t* sample_counts, double* stats, float* pass_films, pt_profile* profile);

/* pt_render_path_exprs (pt_light_groups.h, "Path expressions") under pt_render_adaptive's stop rule, as pt_render_adaptive_path_passes is
 * pt_render_path_passes': film, counts, statistics and rounds are pt_render_adaptive's bit for bit, and expression e's film at pixel p is pt_render_path_exprs' at
 * spp = sample_counts[p].  On success the scene holds the resident FILM and the expression films as its group films, paired. */
pt_status
pt_render_adaptive_path_exprs(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, const pt_path_expr_program* program,
                              const uint8_t* instance_group, uint32_t n_instances, float* film_xyzw, uint32_t* sample_counts, double* stats, float* expr_films,
                              pt_profile* profile);

#ifdef __cplusplus
}
#endif
#endif
