// pt_bin_albedo_device.h — the per-bin albedo fold of one guide sample on the device (pt_render_guides_bin_albedo of include/pt_spectral.h, DESIGN.md
// section 14), shared by the first-hit fold (k_guide_fold_bins, pt_denoise_spectral_albedo.hip) and the chain's terminal vertex (k_chain_step,
// pt_guides_chain.hip).  The rule is pt_denoise_spectral_albedo_rules.h's.
//
// The running sums live in bin-major planes of global memory, sums[b * plane + pixel]: a lane never indexes a register array by a run-time bin number (that
// goes to scratch), neighbouring lanes are neighbouring pixels so every plane access is a coalesced row segment, and the bins are walked in compile-time
// chunks whose eight energies are registers.  Curve values come from the table k_bin_albedo_tables wrote — rows x bins float4, the same address for every
// lane on one surface — so no lane walks a curve.  A chunk fetches each layer's texel again (the same texel: it depends on (u, v) alone); what a layer costs a
// chunk is that fetch and eight table reads.
#ifndef PT_BIN_ALBEDO_DEVICE_H
#define PT_BIN_ALBEDO_DEVICE_H
#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_blob.h"
#include "pt_denoise_spectral_albedo_rules.h"

namespace ptk {

// what the fold needs beside the hit: the sums' planes (`plane` floats each), the table and the first table row of every material's layers
struct BinAlbedoFold { float* sums; const float4* table; const uint32_t* material_row; uint32_t bins, plane; };

// the texture stack of a Lambertian hit: texels from the blob, curve values from the per-bin table
struct BinTableStack {
    const uint32_t* w; const float* tex; const float4* table; uint32_t ts, row, bins; float u, v;
    __device__ uint32_t layers() const { return w[ts]; }
    __device__ ptd::DnTexel texel(uint32_t i) const { return ptd::dn_albedo_texel(w, tex, ts + 1u + i * PT_LAYER_WORDS, u, v); }
    __device__ ptd::DnLayerCurves bin_curves(uint32_t i, uint32_t b) const { const float4 c = table[(size_t)(row + i) * bins + b]; return ptd::DnLayerCurves{c.x, c.y, c.z, c.w}; }
};

// guide sample `h` into the sums of pixel `pixel` (< F.plane): sums[b * plane + pixel] += rho_b for every b < F.bins
__device__ __forceinline__ void bin_albedo_fold_hit(const BinAlbedoFold& F, uint32_t pixel, const pt_hit& h, const uint32_t* __restrict__ blob, const float* __restrict__ tex,
                                                    uint32_t material_count) {
    float* px = F.sums + pixel;
    const uint32_t plane = F.plane;
    auto sum = [&](uint32_t b) -> float& { return px[(size_t)b * plane]; };
    uint32_t mi = 0u, ts = 0u;
    if (ptd::dn_bin_albedo_lambertian_hit(blob, h.valid, h.material, material_count, &mi, &ts)) {
        const BinTableStack stack{blob, tex, F.table, ts, F.material_row[mi], F.bins, h.uv[0], h.uv[1]};
        ptd::dn_bin_albedo_add(&stack, F.bins, sum);
    } else {
        ptd::dn_bin_albedo_add((const BinTableStack*)nullptr, F.bins, sum);
    }
}

}  // namespace ptk
#endif
