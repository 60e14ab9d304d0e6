// pt_forms.h — the names of the kernel forms and the limits and defaults that choose among them.  Plain constants, no HIP: pt_launch.h takes them for the
// launchers, pt_plan.h for the host-side choice (plan_scene, plan_render).
#ifndef PT_FORMS_H
#define PT_FORMS_H
#include <stdint.h>

#include "pt_blob.h"

namespace ptk {

enum { PT_LDS_NONE = 0, PT_LDS_ALL = 1, PT_LDS_CORE = 2 };                 // what stage_scene copies into LDS
enum { PT_SHADE_LEAN = 0, PT_SHADE_NO_ENV = 1, PT_SHADE_FULL = 2, PT_SHADE_MEDIUM = 3 };   // k_shade forms (MEDIUM: k_shade_medium, one wavelength)
enum { PT_FORM_ANY = 0, PT_FORM_WALK = 1, PT_FORM_SWEEP = 2, PT_FORM_POOLED = 3, PT_FORM_PARKED = 4, PT_FORM_PARKED_WALK = 5 };  // traversal kernels (5: the parked kernels over the top-level tree instead of a sweep table)
constexpr int kBlock = 256;
constexpr uint32_t kLdsBlobLimitBytes = 64 * 1024;  // the most LDS a staged blob (or its core section) may take
// The whole blob is staged only while it leaves the CU its occupancy: six workgroups of 24 KB fit the 160 KB.  Measured (tools/lds_mode.sh):
// the 65 KB blob of C3 staged whole leaves two workgroups per CU, 615 Msamples/s; its 6.7 KB core alone, the mesh read through L1/L2,
// 752.  C2's 14 KB blob staged whole: 1519; its 7 KB core alone: 1089 (the sweep reads the triangles of the two boxes for every ray).
constexpr uint32_t kLdsAllLimitBytes = PT_BLOB_LDS_ALL_BYTES;
// The parked kernels in workgroups of 512 / 1024 threads (pt_tuning::park_block) stage the whole blob whatever the other kernels do: two workgroups of
// 512 per CU are four waves per SIMD, and 2 x (72 KB + the waves' lists of live rays) fit the CU's 160 KB.  The gem scene of C3: 66 256 B.
constexpr uint32_t kParkBlobLimitBytes = 72 * 1024;
constexpr uint32_t kLightPrepassMax = 16;   // pt_tuning::light_prepass_max's default: the most lights whose boxes a light-sample ray tests one by one for its bound
constexpr uint32_t kGroupEvictBelow = 32;   // pt_tuning::group_evict_below's default (1 = never)
constexpr uint32_t kTopEvictBelow = 48;   // pt_tuning::top_evict_below's default (1 = never); the check runs behind a leaf test of the while-while walk: G2F k_shadow_parked 2545 (never) / 2314 (16) / 2235 (32) / 2126 (40) / 2108 us (48)
constexpr uint32_t kWalkEvictBelow = 32, kWalkSearchBelow = 16;   // pt_tuning::walk_evict_below's and walk_search_below's defaults
#define PT_TUNE_EXPERIMENT_POOL (1u << 31)   /* a pt_tuning::flags bit of its own, unnamed in the public header (round-4 advisor: bit 3 means PT_TUNE_NO_LIVE_LIST in every build); only a measurement build (-DPT_EXPERIMENTS) sets it and has the kernels it selects */
#ifndef PT_FUSE_HERO
#define PT_FUSE_HERO 1   /* round 4: built without machine LICM the hero fused form needs 111 VGPRs — four waves per SIMD, not three — and wins: C5 1153 -> 1179 (3625 us against 1160 + 2578) */
#endif

}  // namespace ptk
#endif
