/* pt_spectral.h — a wavelength-binned film next to the XYZ film.
 *
 * Not part of pt_api.h: that header is the boundary the oracle shares, and the reference keeps no spectrum.  Exported by libptamd.so (pt_); the
 * rules are also compiled into the host emulation of the tests (ptemu_spectral_*).  The definition is DESIGN.md section 14; in short:
 *
 *   every sample of a render is an energy e at a wavelength lambda (four of each with hero wavelengths).  pt_render_spectral renders what pt_render
 *   renders — film_xyzw is pt_render's, bit for bit — and also adds each sample to bin b(lambda) of its pixel, where with lo, hi the desc's wavelength
 *   bounds and w = (hi - lo) / bins (all f32)
 *       x = (lambda - lo) / w,    b = x < 0 ? 0 : min((uint32_t)x, bins - 1)        (NaN: bin 0)
 *   one wavelength:  S[b(lambda)] += e;      hero wavelengths:  S[b(lambda_k)] += e_k / 4.0f  for k = 0..3 in order.
 *   S is a plain f32 running sum in sample order from 0.0f (no 10-sample phases), independent of how the engine cuts the range into passes.  A whole
 *   range (first_sample 0, sample_count 0 or spp) is divided by (float)spp at its end; a partial range leaves the running sum, as the film does.
 *
 * Units: the mean per-sample energy that fell into the bin.  NOTHING is divided by the bin width: a spectral density is S[b] / w.
 * Layout: bin-major planes, row-major with y = 0 the top row like the film: spectral[b * width * height + y * width + x], f32.  Pixels outside
 * the call's shard stay 0.
 *
 * pt_render_adaptive_spectral is pt_render_adaptive with the same bins: a pixel that took n samples holds the fold of those n samples divided by (float)n,
 * so its bins are pixel p of pt_render_spectral at spp = n, bit for bit.  pt_denoise_spectral filters that film and its bins together: the taps and the
 * edge-stopping weights of every a-trous pass are pt_denoise_film's — they come from the XYZ film, its variance and the guides alone — and each bin plane is
 * averaged with them (csrc/pt_denoise_spectral_rules.h, operation by operation).  The bins have no variance of their own.  pt_denoise_spectral does not
 * demodulate them; pt_denoise_spectral_albedo does, by the per-bin albedo that pt_render_guides_bin_albedo renders (csrc/pt_denoise_spectral_albedo_rules.h).
 *
 * pt_spectral_project develops a spectral film: K weighted sums over the bins of every pixel, the weights a matrix that pt_spectral_response_matrix integrates
 * from response curves (csrc/pt_spectral_project_rules.h); pt_spectral_project_resident develops the bins a scene's last spectral render left on the device.
 *
 * pt_render_spectral_multi and pt_render_adaptive_spectral_multi are the two renders on every device of a node, bit for bit.  The bins are not reduced between
 * the devices: each one packs the planes of its own tiles (csrc/pt_spectral_shard_rules.h) and hands them to the host over its own link, and they stay on it as
 * its part of the scene's resident film, which pt_spectral_project_resident develops shard by shard. */
#ifndef PT_SPECTRAL_H
#define PT_SPECTRAL_H
#include "pt_adaptive.h"
#include "pt_api.h"
#include "pt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SPECTRAL_MAX_BINS 64

typedef struct pt_spectral_desc {
    uint32_t bins;          /* 1 .. PT_SPECTRAL_MAX_BINS */
    uint32_t reserved[3];   /* must be 0 */
} pt_spectral_desc;

/* desc: everything pt_render takes, with the same meaning (shards, sample ranges, phase_samples, hero_wavelengths, medium_aware).
 * film_xyzw: width*height*4 f32, pt_render's film.  spectral: bins*width*height f32, required.  profile (may be NULL): pt_render's counters;
 * kernel_seconds[4] (accumulate) includes the spectral kernel. */
pt_status pt_render_spectral(pt_scene* scene, const pt_render_desc* desc, const pt_spectral_desc* spectral_desc,
                             float* film_xyzw, float* spectral, pt_profile* profile);

/* pt_render_adaptive with a spectral film.  desc, adaptive, film_xyzw, sample_counts (required), stats (may be NULL) and profile: pt_render_adaptive's, with
 * the same conditions; film, counts, stats, the number of rounds and the ray counters are pt_render_adaptive's bit for bit.  spectral: bins*width*height f32,
 * required; pixel p's bins are the plain f32 running sums over its n_p samples in sample order, divided once by (float)n_p when the render finishes.
 * One device: pt_render_adaptive_spectral_multi, below, is the call for several. */
pt_status pt_render_adaptive_spectral(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, const pt_spectral_desc* spectral_desc,
                                      float* film_xyzw, uint32_t* sample_counts, double* stats, float* spectral, pt_profile* profile);

/* pt_render_spectral on every device of device_mask from one blocking call: film_xyzw, spectral and the ray counters of the profile are pt_render_spectral's bit
 * for bit, a partial sample range (first_sample / sample_count) included.  device_mask, pt_tuning::multi_virtual and PT_TUNE_MULTI_RCCL mean what they mean for
 * pt_render_multi (bit d = HIP device d, 0 = all); desc->shard_count must be 0, the call deals the tiles itself.  With one device, no virtual devices and no forced
 * RCCL the call is pt_render_spectral itself; PT_TUNE_MULTI_RCCL alone takes the node path with one shard that is the whole film.  The film travels as
 * pt_render_multi's does.  The bins do not: every device packs the planes of its own tiles, copies them to the host and scatters them into `spectral` from its own
 * host thread; the shards are disjoint and cover the film.  profile (may be NULL): pt_render_multi's; kernel_seconds[5] is the set-up (about 0 on a repeated
 * call), kernel_seconds[6] the film reduce plus the longest device's pack, copy and scatter. */
pt_status pt_render_spectral_multi(pt_scene* scene, const pt_render_desc* desc, const pt_spectral_desc* spectral_desc, uint64_t device_mask,
                                   float* film_xyzw, float* spectral, pt_profile* profile);

/* pt_render_adaptive_spectral on every device of device_mask: film, counts, stats, the number of rounds, the ray counters and the bins are
 * pt_render_adaptive_spectral's bit for bit.  The devices, the mask and the one-device case are pt_render_spectral_multi's; film, counts and statistics travel as
 * pt_render_adaptive_multi's do, the bins as pt_render_spectral_multi's.  kernel_seconds[6]: the rounds' exchanges, the gather and the longest device's pack, copy
 * and scatter. */
pt_status pt_render_adaptive_spectral_multi(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, const pt_spectral_desc* spectral_desc,
                                            uint64_t device_mask, float* film_xyzw, uint32_t* sample_counts, double* stats, float* spectral, pt_profile* profile);

/* pt_denoise_film on film_xyzw (desc, sample_counts, stats, guides_xyzw, out_film_xyzw, out_variance: as pt_denoise_film takes them) and, with the same taps
 * and weights, on the `bins` (1 .. PT_SPECTRAL_MAX_BINS) planes of `spectral` (bins*width*height f32, the layout above).  Pass i, live pixel p, bin b:
 *     sb = 0.0f;  sb = sb + w_q * s_b,i(q) over the taps q that pt_denoise_film's pass takes, in its order;  s_b,i+1(p) = sb / sw
 * with w_q and sw the weights and their sum that the colour of p is averaged with.  A tap that is skipped adds nothing.  A pixel is dead — copied through,
 * film and bins, and never read — when pt_denoise_film calls it dead or when one of its bins is not finite.  Where no pixel is dead through its bins alone,
 * out_film_xyzw and out_variance are pt_denoise_film's bit for bit.  This entry has no albedo form: pt_denoise_spectral_albedo, below, is the one that demodulates.
 * Host arrays in, host arrays out; out_film_xyzw may be film_xyzw and out_spectral may be spectral.  out_variance may be NULL. */
pt_status pt_denoise_spectral(const pt_denoise_desc* desc, uint32_t bins, const float* film_xyzw, const uint32_t* sample_counts, const double* stats,
                              const float* guides_xyzw, const float* spectral, float* out_film_xyzw, float* out_spectral, float* out_variance);

/* The guides of pt_render_guides_albedo — or, with a chain of max_chain > 0, of pt_render_guides_chain — and from the same probes a per-bin albedo: the mean
 * reflectance of the guide samples' surfaces at the centre wavelength of each of the render's `bins` (1 .. PT_SPECTRAL_MAX_BINS) wavelength bins.  With
 * lambda_b = pt_spectral_bin_centres' value for bin b, guide sample k of pixel p gives
 *     rho_b,k = min(texstack_eval(lambda_b, u, v), 1)    at a valid hit of a Lambertian material (the hit pt_render_guides_albedo evaluates its albedo at;
 *                                                        with a chain, the end of the sample's specular chain, where pt_render_guides_chain takes its albedo)
 *     rho_b,k = 1                                        at every other hit, and at a miss
 *     A_b(p)  = (rho_b,0 + ... + rho_b,K-1) / (float)K   the f32 sum in sample order from 0.0f
 * chain: NULL (or max_chain 0) = the first hit.  guides_xyzw (required) and albedo_xyzw (may be NULL): width*height*4 f32, those entries' outputs bit for bit.
 * bin_albedo (required): bins*width*height f32 in the spectral film's layout, bin_albedo[b * width * height + y * width + x]. */
pt_status pt_render_guides_bin_albedo(pt_scene* scene, const pt_render_desc* desc, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t bins,
                                      float* guides_xyzw, float* albedo_xyzw, float* bin_albedo);

/* pt_denoise_spectral with the film demodulated by albedo_xyzw as pt_denoise_film_albedo does it, and the bins by bin_albedo:
 *     before the passes   s_b'(p) = s_b(p) / max(A_b(p), 1e-3f)
 *     the passes          pt_denoise_spectral's, over the demodulated film (its taps and weights are pt_denoise_film_albedo's) and the s_b'
 *     after the last      a live pixel's bins are multiplied by the same max(A_b(p), 1e-3f)
 * A pixel is dead — copied through with its input bits, film and bins, and never read — when pt_denoise_film_albedo calls it dead (pt_denoise_film, with
 * albedo_xyzw NULL), when one of its bins is not finite, or when one is not finite after the division.  albedo_xyzw (may be NULL): width*height*4 f32, every
 * channel finite and >= 0.  bin_albedo (may be NULL): bins*width*height f32, every value finite and >= 0.  Both NULL, or both all ones: pt_denoise_spectral's
 * outputs bit for bit.  bin_albedo NULL alone: the bins are filtered as they are, with the demodulated film's weights.  Where no pixel is dead through its bins
 * alone, out_film_xyzw and out_variance are pt_denoise_film_albedo's bit for bit.  Everything else is as pt_denoise_spectral takes it. */
pt_status pt_denoise_spectral_albedo(const pt_denoise_desc* desc, uint32_t bins, const float* film_xyzw, const uint32_t* sample_counts, const double* stats,
                                     const float* guides_xyzw, const float* albedo_xyzw, const float* spectral, const float* bin_albedo, float* out_film_xyzw,
                                     float* out_spectral, float* out_variance);

/* bin b covers [lo + b*w, lo + (b+1)*w), w = (hi-lo)/bins;
 * centres_nm[b] = lo + ((float)b + 0.5f) * w, from the desc's wavelength bounds (f32).  Host only. */
pt_status pt_spectral_bin_centres(const pt_render_desc* desc, const pt_spectral_desc* spectral_desc, float* centres_nm);

/* An uncompressed scanline OpenEXR file (pt_write_exr's writer) with one FLOAT channel per bin, named after the spectral-EXR convention
 * "S0.<centre>nm" with the centre printed %.6f and its '.' replaced by ',' (S0.565,000000nm), plus R, G, B from linear_rgb (width*height*3, may be
 * NULL) so that ordinary viewers show the picture.  The channel list is in byte-wise name order; the string attributes spectralLayoutVersion = "1.0"
 * and emissiveUnits = "W.m^-2.sr^-1" are added.  spectral: bins*width*height as pt_render_spectral returns it; the centres must be finite and give
 * distinct names.  Host only. */
pt_status pt_write_exr_spectral(const char* path, uint32_t width, uint32_t height, uint32_t bins,
                                const float* centres_nm, const float* spectral,
                                const float* linear_rgb, int32_t colorspace);

/* ---- developing a spectral film: K weighted sums over the bins (csrc/pt_spectral_project_rules.h) ---------------------------------
 *
 * A development projects the bins of every pixel onto K response curves — an observer, a camera's sensitivities, a narrow band, each optionally behind a
 * colour filter.  With M a row-major matrix [K][bins]:
 *     out[k * width * height + p] = fold over b = 0 .. bins-1 ascending of acc = acc + M[k][b] * S_b(p), from acc = 0.0f   (f32, multiply and add separate)
 * Nothing is special-cased: a non-finite bin makes that pixel's outputs non-finite, and a zero weight does not protect against a NaN bin. */
#define PT_SPECTRAL_MAX_RESPONSES 16
#define PT_SPECTRAL_MAX_SUBSAMPLES 16
#define PT_RESPONSE_CIE_X (-1)   /* a response that is no curve: the x, y, z component of the engine's colour-matching fit, xyz_bar(lambda * 10.0f) */
#define PT_RESPONSE_CIE_Y (-2)
#define PT_RESPONSE_CIE_Z (-3)
#define PT_SPECTRAL_NO_FILTER (-1)

/* The matrix of K responses over the `spectral_desc->bins` bins of a render `desc` (its wavelength bounds lo, hi; w = (hi - lo) / (float)bins).  Bin b is sampled
 * at lambda_{b,j} = lo + ((float)b + ((float)j + 0.5f) / (float)subsamples) * w, j = 0 .. subsamples-1 (1 .. PT_SPECTRAL_MAX_SUBSAMPLES; with 1 the bin centre of
 * pt_spectral_bin_centres bit for bit), and
 *     matrix[k * bins + b] = (m = 0.0f;  m = m + r_k(lambda_{b,j}) * f(lambda_{b,j}) for j ascending) / (float)subsamples
 * responses[k] (K of them, 1 .. PT_SPECTRAL_MAX_RESPONSES) is an index into `curves` or one of PT_RESPONSE_CIE_X / _Y / _Z; `filter` is an index into `curves` or
 * PT_SPECTRAL_NO_FILTER, and then the term is r_k alone.  curves / curve_data are in pt_scene_desc's representation (curve_data_floats floats; both may be NULL
 * with curve_count 0); a curve's value has the bits of pt_curve_eval for a scene that holds it.  Nothing is divided by the bin width: S_b is the energy that fell
 * into the bin, so the Y row times the bins estimates what the film's Y sums.  Host only: no scene, no device. */
pt_status pt_spectral_response_matrix(const pt_render_desc* desc, const pt_spectral_desc* spectral_desc, const pt_curve* curves, uint32_t curve_count,
                                      const float* curve_data, uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter,
                                      uint32_t subsamples, float* matrix);

/* The projection above of host planes.  spectral: bins * width * height f32 in pt_render_spectral's layout; matrix: K * bins f32, every entry finite;
 * out: K * width * height f32, plane-major like the bins.  Runs on device 0. */
pt_status pt_spectral_project(uint32_t width, uint32_t height, uint32_t bins, uint32_t K, const float* matrix, const float* spectral, float* out);

/* The same projection of the bins that the scene's last successful spectral render — pt_render_spectral, pt_render_adaptive_spectral or one of their node forms —
 * left on the device: bit for bit pt_spectral_project of the array that render returned, without the bins crossing the bus — the matrix goes up and K planes come
 * back.  After a node render the resident film is the devices' packed shards: the matrix goes to each of them, each develops its own pixels and K planes' worth of
 * them come back over its own link.  matrix: K * bins f32 for that render's bins; out: K * width * height f32 for its size (pt_spectral_resident tells all three).
 * Every spectral render, of either kind, ends the residency of the film before it when it starts.  A scene that has not rendered a spectral film, or whose last
 * spectral render failed, has no resident film and the call fails. */
pt_status pt_spectral_project_resident(pt_scene* scene, uint32_t K, const float* matrix, float* out);

/* Width, height and bins of the scene's resident spectral film; zeros when it has none. */
pt_status pt_spectral_resident(pt_scene* scene, uint32_t* width, uint32_t* height, uint32_t* bins);

#ifdef __cplusplus
}
#endif
#endif /* PT_SPECTRAL_H */
