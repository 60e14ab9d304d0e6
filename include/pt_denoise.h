/* pt_denoise.h — a variance-guided edge-avoiding (a-trous) filter for the film of pt_render_adaptive(_multi).
 *
 * Not part of pt_api.h: that header is the boundary the oracle shares, and the reference has no denoiser.  Exported by libptamd.so (pt_) and by
 * the host emulation of the tests (ptemu_).  The definition is DESIGN.md section 13 and, operation by operation, csrc/pt_denoise_rules.h; in short:
 *
 *   guides     per pixel the mean first-hit normal and distance over camera samples 0 .. guide_samples-1 (pt_camera_samples traced as
 *              pt_intersect traces them); a pixel whose normal sum is 0 is sky
 *   variance   of the pixel's mean Y, from the sample count and the f64 sums S1, S2 the adaptive render returns
 *   a pass     i = 0 .. iterations-1, step 2^i: 25 taps of the B3 spline kernel (3/8, 1/4, 1/16), each weighted by the agreement of the normals
 *              (dot^(2^a)), of the depths (against the depth gradient) and of the Y values (against sigma_luminance x the square root of the
 *              two pixels' 3x3-filtered variances); colours are averaged with w, variances with w^2
 *
 *   albedo     per pixel the mean, over the same camera samples, of the first hit's reflectance as XYZ factors: a Lambertian hit's texture stack at
 *              PT_ALBEDO_WAVELENGTHS wavelengths (clamped to 1 as the material clamps it) weighted by the colour-matching functions and normalised
 *              by their sums; every other hit, and a miss, counts as (1, 1, 1)
 *
 * Pixels with a non-finite film channel or variance are copied through and never read.  The engine, the emulation and a numpy restatement agree
 * bit for bit.  pt_denoise_film does not demodulate albedo: a textured Lambertian surface is protected by the luminance weight alone.
 * pt_denoise_film_albedo does: the film is divided by max(albedo, 1e-3) before the passes (the variance by the square of the Y factor) and
 * multiplied by it afterwards, so that the filter averages irradiance and the texture is put back unfiltered.
 *
 *   chains     pt_render_guides_chain takes the guides and the albedo not at the first hit but at the first vertex that is not mirror-like: a
 *              sample walks on through passthrough boundaries and GGX materials with alpha <= alpha_max (refracting at a dielectric, reflecting
 *              at a metal and on total internal reflection, about the geometric normal, no random number drawn) for at most max_chain vertices;
 *              the distance is the length of the whole path.  csrc/pt_guides_chain_rules.h holds it operation by operation.
 *
 *   mattes     pt_render_mattes runs the same probes as the guide passes (camera samples 0 .. S-1, traced as pt_intersect traces them) and keeps,
 *              per pixel, which instance or material each sample saw: R ranked (key, coverage) pairs, anti-aliased with the jitter and the defocus
 *              of the render.  pt_matte_extract turns selections of keys into coverage masks, pt_write_exr_cryptomatte writes the ranks in the
 *              Cryptomatte layout.  Exact like the guides: the engine, the emulation and a numpy restatement agree bit for bit (the section at the
 *              end of this header). */
#ifndef PT_DENOISE_H
#define PT_DENOISE_H
#include "pt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_denoise_desc {
    uint32_t width, height;
    uint32_t iterations;         /* a-trous passes, step 1, 2, 4, ...; 0 = 5; at most 10 */
    float sigma_luminance;       /* 0 = 4 */
    float sigma_depth;           /* 0 = 1 */
    uint32_t normal_power_log2;  /* the normal weight is dot^(2^a); 0 = 7 (power 128); at most 10 */
    uint32_t device;             /* HIP device the filter runs on (after pt_render_adaptive_multi: the first device of its mask) */
    uint32_t reserved[1];        /* must be 0 */
} pt_denoise_desc;

/* guides_xyzw: width*height*4 f32 = (mean first-hit normal xyz, mean first-hit distance) over camera samples 0 .. guide_samples-1 of `desc`
 * (width, height, seed, wavelength bounds, camera_index; jitter, aperture and camera kind as the render's own first stage has them). */
pt_status pt_render_guides(pt_scene* scene, const pt_render_desc* desc, uint32_t guide_samples, float* guides_xyzw);

/* film_xyzw, sample_counts (every one at least 2), stats: what pt_render_adaptive(_multi) returned for a film of desc->width x desc->height.
 * guides_xyzw: pt_render_guides' output (finite).  out_film_xyzw: width*height*4 f32 (W = 0).  out_variance: width*height f32, the filtered
 * film's variance estimate, may be NULL.  Host arrays in, host arrays out; out_film_xyzw may be film_xyzw. */
pt_status pt_denoise_film(const pt_denoise_desc* desc, const float* film_xyzw, const uint32_t* sample_counts, const double* stats,
                          const float* guides_xyzw, float* out_film_xyzw, float* out_variance);

#define PT_ALBEDO_WAVELENGTHS 16

/* The basis of the albedo for `desc`'s wavelength bounds: lambda = 16 f32 (nm), xyz = 48 f32 (the X, Y and Z weights of the 16 wavelengths, in
 * this order).  Host only: no device is needed. */
pt_status pt_albedo_basis(const pt_render_desc* desc, float* lambda, float* xyz);

/* pt_render_guides with a second output from the same probes: albedo_xyzw = width*height*4 f32 (W = 0).  guides_xyzw is bit for bit
 * pt_render_guides' output. */
pt_status pt_render_guides_albedo(pt_scene* scene, const pt_render_desc* desc, uint32_t guide_samples, float* guides_xyzw, float* albedo_xyzw);

/* pt_denoise_film on the film demodulated by albedo_xyzw (pt_render_guides_albedo's output: every channel finite and >= 0).  A pixel that the
 * division makes non-finite is copied through like any dead pixel.  albedo_xyzw NULL = pt_denoise_film; an albedo of ones gives its output bit
 * for bit. */
pt_status pt_denoise_film_albedo(const pt_denoise_desc* desc, const float* film_xyzw, const uint32_t* sample_counts, const double* stats,
                                 const float* guides_xyzw, const float* albedo_xyzw, float* out_film_xyzw, float* out_variance);

#define PT_GUIDE_CHAIN_MAX 16

typedef struct pt_guide_chain_desc {
    uint32_t max_chain;    /* specular vertices followed per sample; at most PT_GUIDE_CHAIN_MAX; 0 = pt_render_guides_albedo bit for bit */
    float alpha_max;       /* a GGX material with alpha <= alpha_max is specular; 0 = 0.01, which separates the material library's smooth GGX
                              materials (alpha <= 0.004) from its rough ones (>= 0.02) */
    uint32_t reserved[2];  /* must be 0 */
} pt_guide_chain_desc;

/* pt_render_guides_albedo with the guides and the albedo of every sample taken at the end of its specular chain (above).  albedo_xyzw may be
 * NULL: guides_xyzw is the same with and without it.  On a scene without a specular material any max_chain gives pt_render_guides_albedo's
 * outputs bit for bit. */
pt_status pt_render_guides_chain(pt_scene* scene, const pt_render_desc* desc, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                 float* guides_xyzw, float* albedo_xyzw);

/* ---- ID mattes (csrc/pt_matte_rules.h operation by operation) ---- */

enum { PT_MATTE_KEY_INSTANCE = 0, PT_MATTE_KEY_MATERIAL = 1 };
#define PT_MATTE_SKY  0xFFFFFFFEu   /* the key of a sample that hit nothing */
#define PT_MATTE_NONE 0xFFFFFFFFu   /* the key of an empty rank */
#define PT_MATTE_RANKS_MAX 8

typedef struct pt_matte_desc {
    uint32_t samples;      /* S camera samples per pixel, 1 .. 65535 */
    uint32_t ranks;        /* R (key, coverage) pairs kept per pixel, 1 .. PT_MATTE_RANKS_MAX */
    uint32_t key;          /* PT_MATTE_KEY_INSTANCE: pt_hit::instance; PT_MATTE_KEY_MATERIAL: pt_hit::material */
    uint32_t reserved[1];  /* must be 0 */
} pt_matte_desc;

/* The matte of `desc` (width, height, seed, wavelength bounds, camera_index, as pt_render_guides reads them).  keys, coverage: ranks planes of
 * width*height, rank r of pixel p at r*width*height + p, ranked by coverage descending (ties: the smaller key); overflow: width*height u32, the
 * samples whose key found no free rank.  Any output may be NULL: the keys and the coverage stay resident on the scene's device, until the next matte
 * render replaces them; a film render does not touch them. */
pt_status pt_render_mattes(pt_scene* scene, const pt_render_desc* desc, const pt_matte_desc* matte, uint32_t* keys, float* coverage, uint32_t* overflow);

/* The size, ranks and samples of the resident matte; refused before a matte render has succeeded on the scene. */
pt_status pt_mattes_resident(pt_scene* scene, uint32_t* width, uint32_t* height, uint32_t* ranks, uint32_t* samples);

/* out: set_count planes of width*height f32, plane m the coverage of selection m = selected[offsets[m] .. offsets[m+1]-1] (any order, duplicates
 * allowed, PT_MATTE_SKY allowed, may be empty): 0.0f plus, for r ascending, coverage[r] where keys[r] is selected.  set_count <= 16, offsets[0] = 0,
 * offsets[set_count] <= 1024.  Host arrays in and out; runs on HIP device `device`. */
pt_status pt_matte_extract(uint32_t width, uint32_t height, uint32_t ranks, const uint32_t* keys, const float* coverage, uint32_t set_count,
                           const uint32_t* offsets, const uint32_t* selected, uint32_t device, float* out);

/* pt_matte_extract of the resident matte: only the selections go up and set_count planes come back. */
pt_status pt_matte_extract_resident(pt_scene* scene, uint32_t set_count, const uint32_t* offsets, const uint32_t* selected, float* out);

/* The Cryptomatte id of a name: hash = MurmurHash3_x86_32 of its bytes (seed 0); id = the float whose bits are the hash with bit 23 flipped where
 * the exponent field is 0 or 255.  Either output may be NULL.  Host only: no device is needed. */
pt_status pt_cryptomatte_hash(const char* name, uint32_t* hash, float* id);

/* A Cryptomatte file (uncompressed scanline OpenEXR, FLOAT channels): <layer>NN.R/.G/.B/.A for NN = 00 .. ceil(ranks/2)-1 = (id of rank 2NN, its
 * coverage, id of rank 2NN+1, its coverage), an odd last rank padded with 0; R, G, B from linear_rgb (width*height*3) where given.  A key's id is
 * that of its name: names[i] for name_keys[i], else "key<decimal>"; PT_MATTE_SKY and PT_MATTE_NONE are id 0.0f.  The header carries
 * cryptomatte/<7 hex digits of the layer name's hash>/name, /hash, /conversion and /manifest (one entry per name passed).  Host only. */
pt_status pt_write_exr_cryptomatte(const char* path, uint32_t width, uint32_t height, uint32_t ranks, const uint32_t* keys, const float* coverage,
                                   const char* layer, uint32_t name_count, const uint32_t* name_keys, const char* const* names, const float* linear_rgb,
                                   int32_t colorspace);

#ifdef __cplusplus
}
#endif
#endif /* PT_DENOISE_H */
