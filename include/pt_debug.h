/* pt_debug.h — probes of the engine beyond the boundary the oracle shares (include/pt_api.h): entry points for tests of single stages
 * that the reference has no counterpart for.  Exported by libptamd.so (pt_) and by the host emulation of the tests (ptemu_). */
#ifndef PT_DEBUG_H
#define PT_DEBUG_H
#include "pt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Light sampling of one light-list entry (0 .. N-1, World::new's order: an emissive mesh face is an entry of its own) from n points `from` (3 floats each) with
 * sample2d (2 floats each): Hittable::sample through the Instance wrapper (rect.rs:113-173, sphere.rs, disk.rs, instance.rs:134-170; a mesh face: DESIGN.md
 * section 10) — the world direction (3 floats) and the solid-angle pdf, without the pick pdf 1 / N, 0 where it is not finite. */
pt_status pt_light_sample(pt_scene* scene, uint32_t light_entry, size_t n, const float* from, const float* sample2d, float* dir, float* pdf);

#ifdef __cplusplus
}
#endif
#endif
