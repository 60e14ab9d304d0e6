/* pt_resident.h — the adaptive render's film, its bins and the denoiser's guides kept on the device, and the filter and the development run where they lie.
 *
 * Not part of pt_api.h.  Exported by libptamd.so (pt_); the rules of the filter's resident form are also compiled into the host emulation of the tests
 * (csrc/pt_denoise_resident_rules.h, ptemu_).  The definition is DESIGN.md section 14, "The resident filter"; in short:
 *
 *   A scene keeps a resident set on its device.  Its parts (PT_RESIDENT_* bits, pt_resident_info) are
 *     FILM           the film, the sample counts and the statistics (S1, S2) of an adaptive render: always together
 *     BINS           that render's wavelength bins
 *     GUIDES         the filter's guides           ALBEDO   the XYZ albedo           BIN_ALBEDO   the per-bin albedo
 *     DENOISED       the denoised film and its variance            DENOISED_BINS   the denoised bins
 *   A successful one-device pt_render_adaptive or pt_render_adaptive_spectral makes FILM (and BINS) resident.  Every render through pt_render, the adaptive and
 *   spectral entries and their node forms ends the residency of every part when it starts; a node render on more than one device, a plain pt_render and a
 *   failed render leave nothing resident.  pt_resident_guides renders GUIDES (ALBEDO, BIN_ALBEDO) for the resident film, pt_resident_load adopts host arrays
 *   as parts, pt_denoise_resident filters what is resident and leaves DENOISED (DENOISED_BINS), pt_spectral_project_resident_denoised develops those.
 *   An adaptive node render leaves its pieces on the devices — film, counts and statistics on the first device of the mask, the bins as one packed shard per
 *   device — and the scene remembers where: pt_resident_assemble gathers them on the scene's own device, device to device, as FILM (and BINS), so that the
 *   guides and the filter follow a node render as they follow a one-device one.  pt_resident_read copies resident FILM and BINS to host arrays.
 *
 * The contract.  Every output of pt_denoise_resident is bit for bit what the host-array entry — pt_denoise_film, pt_denoise_film_albedo, pt_denoise_spectral
 * or pt_denoise_spectral_albedo, whichever the resident set selects — returns for the arrays the render and guide entries returned; the developed planes are
 * bit for bit pt_spectral_project of those denoised bins.  The filter never writes the render's bins: pt_spectral_project_resident develops the undenoised
 * bins after it as before it, and its meaning (pt_spectral.h) does not change — it is about renders, and nothing in this header makes it succeed or fail. */
#ifndef PT_RESIDENT_H
#define PT_RESIDENT_H
#include "pt_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_RESIDENT_FILM 1u
#define PT_RESIDENT_BINS 2u
#define PT_RESIDENT_GUIDES 4u
#define PT_RESIDENT_ALBEDO 8u
#define PT_RESIDENT_BIN_ALBEDO 16u
#define PT_RESIDENT_DENOISED 32u
#define PT_RESIDENT_DENOISED_BINS 64u

/* (no typedef: the struct shares its name with the entry that fills it, so it is always written `struct pt_resident_info`) */
struct pt_resident_info {
    uint32_t width, height;   /* of every resident part; zeros when nothing is resident */
    uint32_t bins;            /* of BINS, BIN_ALBEDO and DENOISED_BINS; 0 when none of them is resident */
    uint32_t parts;           /* PT_RESIDENT_* bits */
};

/* What the scene holds resident now. */
pt_status pt_resident_info(pt_scene* scene, struct pt_resident_info* info);

/* The guide pipeline of pt_render_guides (flags 0), pt_render_guides_albedo (PT_RESIDENT_ALBEDO) or pt_render_guides_bin_albedo (PT_RESIDENT_ALBEDO |
 * PT_RESIDENT_BIN_ALBEDO, over the resident bins' count) for the render `desc`, its device outputs kept as GUIDES (ALBEDO, BIN_ALBEDO) instead of copied out:
 * they hold the bits those entries return.  `chain` (may be NULL) means what it means for pt_render_guides_bin_albedo: with max_chain > 0 the guides are taken
 * at the end of every sample's specular chain.  desc's width and height must be the resident film's; PT_RESIDENT_BIN_ALBEDO needs PT_RESIDENT_ALBEDO and
 * resident bins.  The parts not asked for, and the denoised parts, are resident no longer. */
pt_status pt_resident_guides(pt_scene* scene, const pt_render_desc* desc, uint32_t guide_samples, const pt_guide_chain_desc* chain, uint32_t flags);

/* Adopts host arrays as resident parts: a film that came from a node render or from disk, or inputs made by hand.  Every pointer may be NULL; a part that is
 * given replaces the resident one, and the denoised parts are resident no longer.  film_xyzw (4 f32 per pixel), sample_counts (u32) and stats (2 f64) come
 * together; spectral and bin_albedo are `bins` planes (1 .. PT_SPECTRAL_MAX_BINS); guides_xyzw and albedo_xyzw are 4 f32 per pixel.  width x height (and bins)
 * must be those of the parts that stay resident.  The values must be what the host-array denoise entries accept: every count at least 2, every guide finite,
 * every albedo finite and not negative.  It does not make a spectral film resident in pt_spectral_project_resident's sense: that entry is about renders. */
pt_status pt_resident_load(pt_scene* scene, uint32_t width, uint32_t height, uint32_t bins, const float* film_xyzw, const uint32_t* sample_counts, const double* stats,
                           const float* spectral, const float* guides_xyzw, const float* albedo_xyzw, const float* bin_albedo);

#define PT_RESIDENT_ASSEMBLE_STAGED 1u   /* copy every shard into staging on the scene's device first, also one that already lies there */

/* Makes FILM, and BINS if the render had bins, resident on the scene's own device from the pieces the last adaptive node render (pt_render_adaptive_multi or
 * pt_render_adaptive_spectral_multi over more than one device, made with stats) left on the devices: bit for bit the arrays that render returned.  Film,
 * counts and statistics are copied from the first device of the mask; every device's packed shard of the bins is unpacked into full planes, in place when it
 * lies on the scene's physical device and through a staging buffer the scene keeps (a peer copy) when it does not.  PT_RESIDENT_ASSEMBLE_STAGED takes the
 * staged route for every shard; both give the same bits.  Nothing but the shards' pixel lists crosses a host link, no peer-access setting is changed, the
 * caller's current device is kept and the call has synchronised when it returns.  The parts lie in pt_resident_load's buffers, never in a render's: the
 * undenoised shards still develop where they are (pt_spectral_project_resident).  GUIDES, ALBEDO, BIN_ALBEDO and the denoised parts are resident no longer.
 * After pt_render_adaptive_light_groups_multi (include/pt_light_groups_multi.h) every device's packed shard of the group films is unpacked the same way, into
 * the buffer a one-device group render leaves them in, and the group films are resident there and paired with the assembled film, as after
 * pt_render_adaptive_light_groups: pt_resident_guides, pt_denoise_light_groups_resident and pt_light_groups_mix_resident(_denoised) follow.
 * A repeated call allocates nothing.  Every render entry forgets the node render when it starts: refused after a later render, after a fixed-count node
 * render, after a node render that came down to one device (it left FILM resident itself) and after a failed one. */
pt_status pt_resident_assemble(pt_scene* scene, uint32_t flags);

/* Copies resident FILM (film_xyzw 4 f32 per pixel, sample_counts u32, stats 2 f64) and BINS (spectral: the resident bins' planes) to host arrays, however they
 * became resident.  Every pointer may be NULL; one that is given for a part that is not resident is refused. */
pt_status pt_resident_read(pt_scene* scene, float* film_xyzw, uint32_t* sample_counts, double* stats, float* spectral);

#define PT_RESIDENT_PLANAR_GATHER 1u   /* pt_resident_denoise_desc::flags: the passes over plane-major bins (pt_denoise_spectral's kernels), not over quads of four bins */

typedef struct pt_resident_denoise_desc {
    pt_denoise_desc filter;   /* width and height: 0 or the resident size; device is ignored: the filter runs where the film is */
    uint32_t flags;           /* PT_RESIDENT_PLANAR_GATHER or 0; both forms give the same bits */
    uint32_t reserved[3];     /* must be 0 */
} pt_resident_denoise_desc;

/* The filter over the resident set.  What runs depends on what is resident alone: BINS — the joint filter; ALBEDO or BIN_ALBEDO — demodulation by it.  FILM and
 * GUIDES are required.  Every out pointer may be NULL, and nothing crosses the bus for a NULL one: out_film_xyzw 4 f32 per pixel, out_variance 1, out_spectral
 * the resident bins' planes (refused without resident bins).  The denoised film, its variance and the denoised bins stay resident (DENOISED, DENOISED_BINS);
 * the sources are not written, so the call may be repeated with other parameters.  Scratch is kept with the scene: a repeated call allocates nothing. */
pt_status pt_denoise_resident(pt_scene* scene, const pt_resident_denoise_desc* desc, float* out_film_xyzw, float* out_variance, float* out_spectral);

/* pt_spectral_project's kernel over the resident denoised bins: out is K * width * height f32, bit for bit pt_spectral_project of the bins pt_denoise_resident
 * returns.  matrix: K * bins f32, every entry finite. */
pt_status pt_spectral_project_resident_denoised(pt_scene* scene, uint32_t K, const float* matrix, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PT_RESIDENT_H */
