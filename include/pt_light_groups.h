/* pt_light_groups.h — light groups: per-group films from one render, mixed on the device.
 *
 * Not part of pt_api.h: that header is the boundary the oracle shares, and the reference keeps one film.  Exported by libptamd.so (pt_); the rules are also
 * compiled into the host emulation of the tests (ptemu_light_groups_*).  The definition is DESIGN.md section 15; in short:
 *
 *   every instance of the scene belongs to one of G groups, 1 <= G <= 8, and so does the environment.  Every addition to a sample's energy goes to the plane of
 *   exactly one group: a light vertex to the group of the instance it lies on (an emissive mesh face: its instance's), an environment vertex to the
 *   environment's, a light-sample ray that hits a light to the group of the instance it hit, an environment light-sample ray that escapes to the environment's.
 *   Within a light-sample item group g's share is the sum in ray order of g's ray contributions, divided by light_samples.  Group g's film is made from group
 *   g's energies as pt_render's is made from all of them: the same wavelengths, phases of 10 and normalisation.
 *
 *   film_xyzw is pt_render's film bit for bit.  Where every film is finite, group g's film is pt_render's of the same scene with every emitter outside g
 *   emitting a zero curve, bit for bit.  Contributions are routed, nothing is multiplied by zero: an infinite factor times a zero emission is NaN in that masked
 *   render and absent here.
 *
 * Layout: group-major films, each row-major like the film with y = 0 the top row: group_films[((g * height + y) * width + x) * 4 + c], f32, w = 0.
 *
 * The mix (the relight): with M[g] a row-major 3 x 3 per group, all f32, no contraction,
 *   out_c(p) = fold over g ascending of acc = acc + ((M[g][c][0] * X_g(p) + M[g][c][1] * Y_g(p)) + M[g][c][2] * Z_g(p)), from acc = 0.0f;   out_w = 0.
 * A scaled identity is a group's intensity, a diagonal its tint, a full matrix a white balance of its own, zero switches it off.
 *
 * The adaptive group render and the joint filter over group films are pt_light_groups_denoise.h's. */
#ifndef PT_LIGHT_GROUPS_H
#define PT_LIGHT_GROUPS_H
#include "pt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_LIGHT_GROUPS_MAX 8

typedef struct pt_light_groups_desc {
    uint32_t group_count;             /* 1 .. PT_LIGHT_GROUPS_MAX */
    uint32_t instance_count;          /* must equal the scene's */
    const uint8_t* instance_group;    /* per instance, each < group_count; read for every instance, used where it emits */
    uint32_t environment_group;       /* < group_count */
    uint32_t reserved[2];             /* must be 0 */
} pt_light_groups_desc;

/* desc: what pt_render takes, one wavelength per path, the plain walk, the whole film and the whole sample range: hero_wavelengths 4, medium_aware, a shard and
 * a partial sample range are PT_ERR_UNSUPPORTED.  film_xyzw: width*height*4 f32, pt_render's film.  group_films: group_count*width*height*4 f32, or NULL when
 * only the resident copy is wanted.  profile (may be NULL): pt_render's counters; kernel_seconds[4] (accumulate) includes the per-group kernel.
 * The group films stay on the scene's device until the next group render replaces them or the scene is destroyed. */
pt_status pt_render_light_groups(pt_scene* scene, const pt_render_desc* desc, const pt_light_groups_desc* groups, float* film_xyzw, float* group_films,
                                 pt_profile* profile);

/* The mix of host arrays.  group_films: group_count*width*height*4 f32; matrices: group_count*9 f32, row-major, every entry finite; out_xyzw: width*height*4 f32.
 * width x height within 31 bits. */
pt_status pt_light_groups_mix(uint32_t width, uint32_t height, uint32_t group_count, const float* group_films, const float* matrices, float* out_xyzw);

/* What the scene's last group render left on its device: its size and group count, or three zeros when there is none. */
pt_status pt_light_groups_resident(pt_scene* scene, uint32_t* width, uint32_t* height, uint32_t* group_count);

/* pt_light_groups_mix over the resident group films: the matrices go up, one film comes back. */
pt_status pt_light_groups_mix_resident(pt_scene* scene, const float* matrices, float* out_xyzw);

#ifdef __cplusplus
}
#endif
#endif
