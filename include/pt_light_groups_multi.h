/* pt_light_groups_multi.h — light groups on every device of a node: the fixed and the adaptive group render sharded by tiles, the group films packed and
 * relit per device.  The third part of the light-group surface; pt_light_groups.h and pt_light_groups_denoise.h keep the one-device entries as they are.
 * Exported by libptamd.so (pt_); the packed shard's rule and the argument checks are also compiled into the host emulation of the tests
 * (tests/host_emulation/ptemu_light_groups_shard.cpp).  The definition is DESIGN.md section 15, "On every device of a node"; in short:
 *
 *   The film's tiles are dealt to the devices of the mask as pt_render_multi deals them.  Every device renders its own tiles into a film and G group films of
 *   its own.  Film, counts and statistics are gathered on the first device of the mask as pt_render_multi and pt_render_adaptive_multi gather them.  The group
 *   films are never reduced: every device packs the pixels of its own tiles, packed[g * n_own + i] = group film g at pixel px[i] (px: the shard's pixel list,
 *   n_own entries), hands G * n_own * 16 bytes to the host itself, where its own thread writes them into the caller's array, and keeps the packed shard as
 *   its part of the scene's resident group films.  Every pixel is in exactly one shard, so every pixel of the caller's array is written exactly once.
 *
 * device_mask, pt_tuning::multi_virtual and PT_TUNE_MULTI_RCCL mean what they mean for pt_render_multi.  One device without virtual devices and without the
 * forced RCCL path is the one-device call itself, with everything that call leaves resident.
 *
 * After a node call over more than one (virtual) device the resident group films are the packed shards: pt_light_groups_resident reports their size and
 * count, and pt_light_groups_mix_resident uploads the matrices to every device that holds a shard, mixes the shard where it lies and scatters n_own pixels per
 * device — bit for bit pt_light_groups_mix of the returned array.  The resident film is ended and the group films are paired with none, so
 * pt_denoise_light_groups_resident and pt_light_groups_mix_resident_denoised refuse until pt_resident_assemble (include/pt_resident.h) has gathered the pieces of an
 * adaptive node group render on the scene's own device.  Either kind of group call ends the residency of the group films before it, and a refused node call
 * leaves none. */
#ifndef PT_LIGHT_GROUPS_MULTI_H
#define PT_LIGHT_GROUPS_MULTI_H
#include "pt_light_groups_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pt_render_light_groups on every device of the mask (0 = all) from one blocking call: film_xyzw, group_films (may be NULL: the shards stay resident, nothing
 * of them crosses a host link) and the five ray counters of the profile are pt_render_light_groups', bit for bit.  Refused is what that entry refuses, with
 * its words, except that a shard in the desc is this entry's own refusal (PT_ERR_INVALID_ARGUMENT: the call deals the tiles itself, shard_count must be 0).
 * profile (may be NULL): pt_render_multi's; kernel_seconds[5] is the set-up (about 0 on a repeated call), kernel_seconds[6] the gather plus the longest
 * worker's pack, copy and scatter. */
pt_status pt_render_light_groups_multi(pt_scene* scene, const pt_render_desc* desc, const pt_light_groups_desc* groups, uint64_t device_mask, float* film_xyzw,
                                       float* group_films, pt_profile* profile);

/* pt_render_adaptive_light_groups on every device of the mask: film_xyzw, sample_counts, stats (may be NULL), group_films (may be NULL), the rounds and the ray
 * counters are that entry's, bit for bit; the rounds run in lockstep as pt_render_adaptive_multi's do.  Refused is what that entry refuses, the shard as above.
 * Made with stats over more than one (virtual) device, the render is one pt_resident_assemble can gather: FILM on the scene's device, and the group films
 * unpacked beside it and paired with it, as after pt_render_adaptive_light_groups. */
pt_status pt_render_adaptive_light_groups_multi(pt_scene* scene, const pt_render_desc* desc, const pt_adaptive_desc* adaptive, const pt_light_groups_desc* groups,
                                                uint64_t device_mask, float* film_xyzw, uint32_t* sample_counts, double* stats, float* group_films,
                                                pt_profile* profile);

#ifdef __cplusplus
}
#endif
#endif
