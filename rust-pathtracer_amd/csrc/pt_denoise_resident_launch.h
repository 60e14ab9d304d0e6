// pt_denoise_resident_launch.h — the filter's run on device pointers (pt_denoise.hip): what the four host-array entries run between their upload and their
// read-back, and what pt_denoise_resident (pt_engine.hip, where pt_scene lives) runs on the scene's resident buffers.  Every pointer is device memory of the
// current device.
#ifndef PT_DENOISE_RESIDENT_LAUNCH_H
#define PT_DENOISE_RESIDENT_LAUNCH_H
#include <hip/hip_runtime.h>

#include "../../include/pt_denoise.h"

namespace ptk {

// One run of the filter over width x height pixels (np) and `bins` planes of them.  What runs depends on which inputs are present alone.
struct DnRun {
    // inputs, never written (out_film may be film: the finish is one lane per pixel, in place)
    const float* film; const uint32_t* counts; const double* stats; const float* guides;   // np float4, np, np double2, np float4
    const float* albedo;       // np float4, or null
    uint32_t bins;             // 0: the film filter
    const float* spectral;     // bins planes, or null.  Where it is bin_buf[0] the bins are tested where they lie (no albedo of either kind); elsewhere they are
                               // divided, or copied through the dead test of the division, into bin_buf[0] (with quads: into the quads of bin_buf[0])
    const float* bin_albedo;   // bins planes, or null
    // scratch
    float* color[2]; float* geo; float* tent; uint8_t* flags; float* grad;   // np float4 x 2, np float4, np, np bytes, np float2
    float* bin_buf[2];         // the passes' ping-pong buffers: bins planes each; with quads dn_quad_count(bins) planes of float4 each
    // The bins between the passes as quads (pt_denoise_resident_rules.h): k_dn_bins_to_quads, k_dn_gather_spectral_quad per pass and k_dn_quads_to_bins
    // into out_bins (bins planes; neither bin_buf, nor spectral).  Without: the plane-major kernels, and the denoised bins are left in a bin_buf.
    bool quads; float* out_bins;
    // outputs
    float* out_film; float* out_variance;   // np float4, np
    const float* denoised_bins;             // set by dn_run: where the denoised bins lie, plane-major (out_bins, or a bin_buf)
    // Light-group films beside the film (pt_denoise_light_groups_rules.h; never together with bins): `groups` group-major float4 films of np pixels.  group_films
    // is read only; group_buf are the passes' ping-pong buffers, groups * np float4 each; out_groups takes the denoised films (it may be group_films: the finish
    // runs after the last read of them, one lane per pixel).  groups 0: none of this is looked at.
    uint32_t groups; const float* group_films; float* group_buf[2]; float* out_groups;
};
// the launches of one run of the normalised descriptor `d` on `stream`; nothing is synchronised
void dn_run(const pt_denoise_desc& d, DnRun* run, hipStream_t stream);
// scratch sizes in bytes for np pixels
inline size_t dn_bin_buf_bytes(size_t np, uint32_t bins, bool quads) { return quads ? 16 * np * ((bins + 3u) / 4u) : 4 * np * bins; }

}  // namespace ptk
#endif
