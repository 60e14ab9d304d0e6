// pt_guides_chain.hip — the denoiser guides that follow specular chains (include/pt_denoise.h pt_render_guides_chain) on gfx950.
// Per sample index: k_chain_rays writes the camera rays of every pixel with the identity pixel list; then, per chain vertex, the closest-hit probe runs
// over the rays still on their way and k_chain_step, one lane per ray, applies pt_guides_chain_rules.h to the 52-byte hit record.  A ray that ends folds into
// its pixel's sums — a pixel owns one ray per sample index and the launches of a stream run in order, so the fold needs no atomic and its order is the
// sample order.  A ray that goes on is appended to the next vertex' list: a wave ballot, the count of the lanes below, one atomic add per wave.  The
// order of that list differs from run to run; no output depends on it, since every ray carries its pixel.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"   /* first, as in pt_engine.hip: stage_generate is compiled as the render's own first stage is */
#include "pt_guides_chain_launch.h"
#include "pt_guides_chain_rules.h"

using namespace ptd;

namespace {

constexpr int kLine = 256;
inline uint32_t line_grid(size_t n) { return (uint32_t)((n + kLine - 1) / kLine); }

__global__ void __launch_bounds__(kLine) k_chain_rays(RenderParams rp, uint32_t n, uint32_t sample, float* __restrict__ o, float* __restrict__ d, uint4* __restrict__ state) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PathVertexT<1> p = stage_generate<1>(rp, sample, i);   // (chunk_pixels 1: the slot is the sample index, as in pt_camera_samples)
    o[3 * i] = p.o.x; o[3 * i + 1] = p.o.y; o[3 * i + 2] = p.o.z;
    d[3 * i] = p.d.x; d[3 * i + 1] = p.d.y; d[3 * i + 2] = p.d.z;
    state[i] = make_uint4(i, pt_f2u(p.lambda), pt_f2u(0.0f), 0u);
}

// the texture stack of a Lambertian hit: texels from the blob, curve values from the table k_albedo_tables wrote (pt_denoise.hip)
struct TableStack {
    const uint32_t* w; const float* tex; const float4* table; uint32_t ts, row; float u, v;
    __device__ uint32_t layers() const { return w[ts]; }
    __device__ DnTexel texel(uint32_t i) const { return dn_albedo_texel(w, tex, ts + 1u + i * PT_LAYER_WORDS, u, v); }
    __device__ DnLayerCurves curves(uint32_t i, int j) const { const float4 c = table[(row + i) * DN_ALBEDO_WAVELENGTHS + (uint32_t)j]; return DnLayerCurves{c.x, c.y, c.z, c.w}; }
};

// (ALBEDO false: no albedo sum is kept and the table is never read; BINS: the per-bin albedo's sums are folded too, pt_bin_albedo_device.h)
template <bool ALBEDO, bool BINS>
__global__ void __launch_bounds__(kLine) k_chain_step(uint32_t n, const pt_hit* __restrict__ hits, const float* __restrict__ d_in, const uint4* __restrict__ state_in,
                                                     float* __restrict__ o_out, float* __restrict__ d_out, uint4* __restrict__ state_out, uint32_t* __restrict__ count_out,
                                                     DnGuideSum* __restrict__ sums, float4* __restrict__ asums, uint32_t vertex, uint32_t max_chain, float alpha_max,
                                                     const uint32_t* __restrict__ blob, const float* __restrict__ tex, uint32_t material_count,
                                                     const uint32_t* __restrict__ material_row, const float4* __restrict__ table, DnAlbedoBasis B, ptk::BinAlbedoFold bin_fold) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool follows = false;
    DnChainNext next;
    uint4 st = make_uint4(0u, 0u, 0u, 0u);
    if (i < n) {   // (no early return: every lane of the wave takes part in the ballot below)
        const pt_hit h = hits[i];
        st = state_in[i];
        float length = pt_u2f(st.z);
        if (h.valid) {
            length = length + h.t;
            const SceneView s{blob, tex, blob + blob[PT_HDR_CORE_WORDS]};
            follows = dn_chain_vertex(s, material_count, h.material, f3(h.point[0], h.point[1], h.point[2]), f3(h.normal[0], h.normal[1], h.normal[2]), h.uv[0], h.uv[1],
                                      f3(d_in[3 * i], d_in[3 * i + 1], d_in[3 * i + 2]), pt_u2f(st.y), alpha_max, vertex, max_chain, &next);
        }
        st.z = pt_f2u(length);
        if (!follows) {   // the sample ends here: a miss, or the terminal vertex
            const uint32_t p = st.x;
            DnGuideSum g = sums[p];
            dn_guide_add(&g, h.valid, length, h.normal[0], h.normal[1], h.normal[2]);
            sums[p] = g;
            if (ALBEDO) {
                DnAlbedo a{1.0f, 1.0f, 1.0f};
                if (dn_albedo_has_record(h.valid, h.material, material_count)) {
                    const uint32_t mi = PT_MATERIAL_INDEX(h.material), m = blob[PT_HDR_MATERIAL_OFF] + mi * PT_MAT_WORDS;
                    if (blob[m + PT_MAT_KIND] == (uint32_t)PT_MATERIAL_LAMBERTIAN)
                        a = dn_albedo_lambertian(TableStack{blob, tex, table, blob[m + PT_MAT_TEXSTACK], material_row[mi], h.uv[0], h.uv[1]}, B);
                }
                const float4 a4 = asums[p];
                DnAlbedo as{a4.x, a4.y, a4.z};
                dn_albedo_add(&as, a);
                asums[p] = make_float4(as.x, as.y, as.z, 0.0f);
            }
            if (BINS) ptk::bin_albedo_fold_hit(bin_fold, p, h, blob, tex, material_count);   // (p < bin_fold.plane: a ray's pixel is one of the film's)
        }
    }
    // the next vertex' list: the wave's rays that go on take consecutive places from the one its first lane reserves
    const unsigned long long mask = __ballot(follows);
    if (mask == 0ull) return;   // (wave-uniform)
    uint32_t start = 0;
    if (ptk::lane_id() == 0) start = atomicAdd(count_out, (uint32_t)__popcll(mask));
    start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
    if (follows) {
        const uint32_t q = start + (uint32_t)__popcll(mask & ((1ull << ptk::lane_id()) - 1ull));   // q < n: at most the n rays of this launch go on
        o_out[3 * q] = next.o.x; o_out[3 * q + 1] = next.o.y; o_out[3 * q + 2] = next.o.z;
        d_out[3 * q] = next.d.x; d_out[3 * q + 1] = next.d.y; d_out[3 * q + 2] = next.d.z;
        state_out[q] = st;
    }
}

}  // namespace

namespace ptk {

void launch_chain_rays(const RenderParams& rp, uint32_t n_pixels, uint32_t sample, const ChainRays& out) {
    hipLaunchKernelGGL(k_chain_rays, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, rp, n_pixels, sample, out.o, out.d, out.state);
}

void launch_chain_step(uint32_t n, const pt_hit* hits, const ChainRays& in, const ChainRays& out, uint32_t* count_out, DnGuideSum* sums, const ChainAlbedo& albedo,
                       uint32_t vertex, uint32_t max_chain, float alpha_max, const uint32_t* blob, const float* tex, uint32_t material_count) {
    if (n == 0) return;
    if (albedo.albedo_sums && albedo.bin_fold.sums)
        hipLaunchKernelGGL((k_chain_step<true, true>), dim3(line_grid(n)), dim3(kLine), 0, 0, n, hits, in.d, in.state, out.o, out.d, out.state, count_out, sums,
                           reinterpret_cast<float4*>(albedo.albedo_sums), vertex, max_chain, alpha_max, blob, tex, material_count, albedo.material_row,
                           reinterpret_cast<const float4*>(albedo.table), albedo.basis, albedo.bin_fold);
    else if (albedo.albedo_sums)
        hipLaunchKernelGGL((k_chain_step<true, false>), dim3(line_grid(n)), dim3(kLine), 0, 0, n, hits, in.d, in.state, out.o, out.d, out.state, count_out, sums,
                           reinterpret_cast<float4*>(albedo.albedo_sums), vertex, max_chain, alpha_max, blob, tex, material_count, albedo.material_row,
                           reinterpret_cast<const float4*>(albedo.table), albedo.basis, albedo.bin_fold);
    else
        hipLaunchKernelGGL((k_chain_step<false, false>), dim3(line_grid(n)), dim3(kLine), 0, 0, n, hits, in.d, in.state, out.o, out.d, out.state, count_out, sums,
                           (float4*)nullptr, vertex, max_chain, alpha_max, blob, tex, material_count, (const uint32_t*)nullptr, (const float4*)nullptr, albedo.basis, albedo.bin_fold);
}

}  // namespace ptk
