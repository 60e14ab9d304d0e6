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
 * the call's shard stay 0. */
#ifndef PT_SPECTRAL_H
#define PT_SPECTRAL_H
#include "pt_api.h"

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

#ifdef __cplusplus
}
#endif
#endif /* PT_SPECTRAL_H */
