/* pt_adaptive.h — adaptive sampling between RenderSettings::min_samples and max_samples (src/parsing/config.rs:53-54).
 *
 * Not part of pt_api.h: that header is the boundary the oracle shares, and the reference has no adaptive tiled renderer.  Exported by
 * libptamd.so (pt_) and by the host emulation of the tests (ptemu_).  The definition is DESIGN.md section 12; in short:
 *
 *   round 0 renders samples [0, spp) of every pixel of the film; round k renders the next `step` samples (at most up to max_samples) of
 *   the pixels still active.  After a round a pixel p with n samples, S1 = sum y and S2 = sum y^2 (y = the Y term the film sum adds,
 *   summed in f64 in sample order) is converged when
 *       (n * S2 - S1 * S1) <= (n - 1) * M * M,    M = max(rel_error * S1, abs_error * n)      (all f64; NaN = not converged)
 *   and stays active while n < max_samples and some pixel of its 3x3 neighbourhood was active and not converged.
 *
 * Every pixel of the result equals, bit for bit, pixel p of pt_render with spp = n_p: rounds start on the 10-sample phase boundaries and
 * the film sums keep the fixed render's order. */
#ifndef PT_ADAPTIVE_H
#define PT_ADAPTIVE_H
#include "pt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_adaptive_desc {
    uint32_t max_samples;   /* the ceiling (RenderSettings::max_samples); desc->spp is the floor (min_samples) */
    uint32_t step;          /* samples added to a still-active pixel per round; 0 = spp */
    float rel_error;        /* target standard error of the pixel's mean Y, relative to that mean */
    float abs_error;        /* ... or absolute, in film Y units, whichever is larger; 0 = purely relative */
} pt_adaptive_desc;

/* desc: phase_samples 0 or 10, spp / step / max_samples multiples of 10 with max_samples >= spp, the whole sample range (first_sample 0,
 * sample_count 0) and the whole film (shard_count 0).  film_xyzw: width*height*4 f32 as pt_render's, pixel p divided by its own count.
 * sample_counts: width*height u32, required.  stats: width*height*2 f64 (S1, S2 per pixel), may be NULL.  profile->camera_rays is the sum of
 * the counts, profile->seconds the whole call; profile->kernel_launches[5] holds the number of rounds. */
pt_status pt_render_adaptive(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive,
                             float* film_xyzw, uint32_t* sample_counts, double* stats, pt_profile* profile);

/* pt_render_adaptive on every device of device_mask, from one blocking call: the mask means what it means for pt_render_multi (0 = every visible
 * device; a mask that names none is refused), and the call deals the film's tiles to the devices itself (desc->shard_count 0).  The rounds run in
 * lockstep: after each round the devices' unconverged images are merged into the film-wide one, so film, sample_counts, stats
 * and the number of rounds equal pt_render_adaptive's bit for bit, and the ray counters sum to its.  profile->kernel_seconds[5] is the set-up,
 * [6] the rounds' exchanges plus the final gather.  With one device (no pt_tuning::multi_virtual, no PT_TUNE_MULTI_RCCL) it is pt_render_adaptive. */
pt_status pt_render_adaptive_multi(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, uint64_t device_mask,
                                   float* film_xyzw, uint32_t* sample_counts, double* stats, pt_profile* profile);

#ifdef __cplusplus
}
#endif
#endif /* PT_ADAPTIVE_H */
