/* pt_light_groups_spectral.h — spectral light groups: the wavelength bins of every light group from one render, and a re-lamp of the finished render.
 *
 * Not part of pt_api.h, pt_light_groups.h or pt_spectral.h, which stay as they are.  Exported by libptamd.so (pt_); the rules are also compiled into the host
 * emulation of the tests (ptemu_, tests/host_emulation/ptemu_light_groups_spectral.cpp).  The definition is DESIGN.md section 15; in short:
 *
 *   Emission enters a sample's energy as one factor, the emission curve at the sample's wavelength, and the walk never looks at an emission value.  A sample of
 *   group g rendered with curve `old` is therefore the sample under curve `new` times new(lambda) / old(lambda): the paths, MIS weights and roulette decisions
 *   stay.  With the bins kept per group a re-lamp is a development of the G * bins planes by a matrix that holds those ratios — up to how far the ratio varies
 *   inside a bin, the re-render with the same seed.
 *
 * The render.  film_xyzw, group_films and the ray counters are pt_render_light_groups' bit for bit, `spectral` is pt_render_spectral's bit for bit.  Group g's
 * bins of a pixel are the f32 running sum, in sample order from 0.0f, of that pixel's group-g energies (pt_light_groups.h), each added to bin
 * spectral_bin(lo, span, bins, lambda) of its sample's wavelength (pt_spectral.h), divided once by (float)spp when the range ends
 * (csrc/pt_light_groups_spectral_rules.h lg_spectral_fold_pixel).  Where every film is finite, group g's bins are pt_render_spectral's bins of the same scene with
 * every emitter outside g emitting a zero curve, bit for bit.
 *
 * Layout of group_spectral: group-major, then bin-major, then the film's rows with y = 0 the top row: group_spectral[((g * bins + b) * height + y) * width + x], f32.
 *
 * The re-lamp: with W a row-major matrix [K][G * bins] and S_i plane i = g * bins + b of group_spectral,
 *     out[k * width * height + p] = fold over i = 0 .. G * bins - 1 ascending of acc = acc + W[k][i] * S_i(p), from acc = 0.0f   (f32, multiply and add separate)
 * — pt_spectral_project's rule with G * bins (at most 512) planes in the place of bins. */
#ifndef PT_LIGHT_GROUPS_SPECTRAL_H
#define PT_LIGHT_GROUPS_SPECTRAL_H
#include "pt_light_groups.h"
#include "pt_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_RELAMP_KEEP (-1)   /* old_curve[g], new_curve[g]: group g keeps its lamp */

/* desc, groups: what pt_render_light_groups takes, under its conditions (one wavelength per path, the plain walk, the whole film and the whole sample range,
 * group_count <= PT_LIGHT_GROUPS_MAX, width x height within 31 bits); spectral_desc: bins in 1 .. PT_SPECTRAL_MAX_BINS.  film_xyzw: width*height*4 f32.
 * group_films (may be NULL): group_count*width*height*4 f32.  spectral (may be NULL): bins*width*height f32.  group_spectral (may be NULL):
 * group_count*bins*width*height f32.  profile (may be NULL): pt_render's counters; kernel_seconds[4] (accumulate) includes the group-bin kernel.
 * The group bins stay on the scene's device as its resident group bins until the next group render of any kind starts (pt_render_light_groups and
 * pt_render_adaptive_light_groups leave none) or the scene is destroyed; the total bins and the group films become the resident spectral film and the resident
 * group films, as after pt_render_spectral and pt_render_light_groups.  The device holds group_count*bins*width*height*4 bytes for them (2 GiB at 1024 x 1024,
 * 8 groups, 64 bins); where that cannot be reserved the call fails with PT_ERR_OUT_OF_MEMORY and the scene stays usable. */
pt_status pt_render_light_groups_spectral(pt_scene* scene, const pt_render_desc* desc, const pt_light_groups_desc* groups, const pt_spectral_desc* spectral_desc,
                                          float* film_xyzw, float* group_films, float* spectral, float* group_spectral, pt_profile* profile);

/* Width, height, group count and bins of the scene's resident group bins; four zeros when it has none. */
pt_status pt_light_groups_spectral_resident(pt_scene* scene, uint32_t* width, uint32_t* height, uint32_t* group_count, uint32_t* bins);

/* The matrix of a re-lamp: K responses over the group_count * bins planes of a render `desc` with `spectral_desc`.  lambda_{b,j}, r_k, the filter f and
 * subsamples n are pt_spectral_response_matrix's, and so are curves / curve_data.  The ratio of group g at a wavelength is
 *     q_g(lambda) = 1.0f                                              when old_curve[g] == PT_RELAMP_KEEP
 *     q_g(lambda) = o > 0.0f ? new(lambda) / o : 0.0f, o = old(lambda)  otherwise (old = curves[old_curve[g]], new = curves[new_curve[g]])
 * and   matrix[(k * group_count + g) * bins + b] = gain[g] * ((m = 0.0f;  m = m + t_k(lambda_{b,j}) * q_g(lambda_{b,j}) for j ascending) / (float)n)
 * with t_k = r_k, or r_k * f behind a filter; all f32, in the order written, no contraction.  gain (may be NULL = all 1.0f): one finite factor per group.
 * With KEEP and gain 1 a group's rows are pt_spectral_response_matrix's bit for bit.
 * q_g is the ratio of EMISSION CURVES: a group whose emitters do not share one emission curve has no single `old`, and neither has an environment whose
 * emission is driven by an HDR texture; such a group can be kept or scaled, not re-lamped.  That is the caller's to avoid.
 * Refused, each with a message of its own: a gain that is not finite, a matrix entry that is not finite, a curve index out of range, new_curve[g] equal to
 * PT_RELAMP_KEEP where old_curve[g] is not.  Host only: no scene, no device. */
pt_status pt_light_groups_relamp_matrix(const pt_render_desc* desc, const pt_spectral_desc* spectral_desc, const pt_curve* curves, uint32_t curve_count,
                                        const float* curve_data, uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter,
                                        uint32_t subsamples, uint32_t group_count, const int32_t* old_curve, const int32_t* new_curve, const float* gain,
                                        float* matrix);

/* The re-lamp of host planes.  group_spectral: group_count * bins * width * height f32 in the render's layout; matrix: K * group_count * bins f32, every entry
 * finite, K in 1 .. PT_SPECTRAL_MAX_RESPONSES; out: K * width * height f32, plane-major.  width x height within 31 bits.  Runs on device 0. */
pt_status pt_light_groups_relamp(uint32_t width, uint32_t height, uint32_t group_count, uint32_t bins, uint32_t K, const float* matrix,
                                 const float* group_spectral, float* out);

/* The same re-lamp of the scene's resident group bins: bit for bit pt_light_groups_relamp of the array the render returned.  K * group_count * bins floats go
 * up and K planes come back; the group bins never cross the bus.  A scene without resident group bins refuses. */
pt_status pt_light_groups_relamp_resident(pt_scene* scene, uint32_t K, const float* matrix, float* out);

#ifdef __cplusplus
}
#endif
#endif
