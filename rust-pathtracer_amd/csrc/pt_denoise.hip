// pt_denoise.hip — the film denoiser of include/pt_denoise.h on gfx950: the kernels of the guide pass (camera rays of one
// sample index for every pixel, the fold of the closest-hit probe's records, the final division) and of the filter (prepare, and per a-trous pass
// the 3x3 variance tent and the 25-tap gather over ping-pong buffers), of the albedo guide (curve tables, the fold and the division with a second
// sum), and pt_denoise_film(_albedo) itself.  Every per-pixel rule is pt_denoise_rules.h's, the text the host emulation compiles, so the outputs
// agree with it bit for bit.
// The filter's launches are ptk::dn_run, on device pointers: the host-array entries run it between an upload and a read-back, pt_denoise_resident
// (pt_engine.hip) on the buffers the scene keeps, where the bins may lie in quads of four between the passes (pt_denoise_resident_rules.h).
//
// One workgroup = one film tile of 32x8 pixels, one pixel per lane (a wave = two rows of 32 pixels: 512 contiguous bytes per float4 plane and row).  The
// gather reads each input 25 times, from L1 / L2 / the Infinity Cache: it is bound by its arithmetic (about 200 vector instructions per tap: two correctly
// rounded divisions, a square root, two pt_exp), not by those reads — a form that staged the tile and its halo in LDS for steps 1, 2 and 4 measured 103, 104
// and 113 us per pass at 1024x1024 against 110 us for this one and is not kept (profiles/denoise_kernel_stats.csv, profiles/patches/denoise_staged_tile.diff).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "pt_kernels.h"   /* first, as in pt_engine.hip: stage_generate is compiled as the render's own first stage is */
#include "../../include/pt_denoise.h"
#include "../../include/pt_spectral.h"
#include "pt_denoise_launch.h"
#include "pt_denoise_resident_launch.h"
#include "../../include/pt_light_groups_denoise.h"
#include "pt_denoise_light_groups_rules.h"
#include "pt_denoise_resident_rules.h"
#include "pt_denoise_rules.h"
#include "pt_denoise_spectral_albedo_rules.h"
#include "pt_error.h"
#include "pt_plan.h"

using namespace ptd;

namespace {

constexpr int kLine = 256;              // the one-dimensional kernels
constexpr int kTileW = 32, kTileH = 8;  // the tent and the gather

pt_status dfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }

// ---------------------------------------------------------------------------------------------- guide pass
__global__ void __launch_bounds__(kLine) k_guide_rays(RenderParams rp, uint32_t n, uint32_t sample, float* __restrict__ o, float* __restrict__ d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PathVertexT<1> p = stage_generate<1>(rp, sample, i);   // (chunk_pixels 1: the slot is the sample index, as in pt_camera_samples)
    o[3 * i] = p.o.x; o[3 * i + 1] = p.o.y; o[3 * i + 2] = p.o.z;
    d[3 * i] = p.d.x; d[3 * i + 1] = p.d.y; d[3 * i + 2] = p.d.z;
}
__global__ void __launch_bounds__(kLine) k_guide_fold(uint32_t n, const pt_hit* __restrict__ hits, DnGuideSum* __restrict__ sums, int first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DnGuideSum g;
    if (first) { g.nx = 0.0f; g.ny = 0.0f; g.nz = 0.0f; g.z = 0.0f; g.hits = 0u; } else g = sums[i];
    const pt_hit h = hits[i];
    dn_guide_add(&g, h.valid, h.t, h.normal[0], h.normal[1], h.normal[2]);
    sums[i] = g;
}
__global__ void __launch_bounds__(kLine) k_guide_finish(uint32_t n, const DnGuideSum* __restrict__ sums, uint32_t samples, float4* __restrict__ guides) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DnGeo g = dn_guide_finish(sums[i], samples);
    guides[i] = make_float4(g.nx, g.ny, g.nz, g.z);
}

// The albedo guide.  k_albedo_tables: one lane per (texture layer of a Lambertian material, basis wavelength j) evaluates the layer's curves once per call, so
// that no lane of the fold walks a curve.  k_guide_fold_albedo: k_guide_fold plus the albedo sum from the same 52-byte hit record; a Lambertian hit fetches its
// layers' texels once and runs the 16 wavelengths over the table (16 B per layer and wavelength, the same address for every lane on one surface: L1 hits).  The
// basis comes in the kernel arguments: its weights are scalar operands of the unrolled loop.
static_assert(DN_ALBEDO_WAVELENGTHS == PT_ALBEDO_WAVELENGTHS, "the rules' basis is the header's");
__global__ void __launch_bounds__(kLine) k_albedo_tables(const uint32_t* __restrict__ blob, const float* __restrict__ tex, DnAlbedoBasis B, uint32_t rows,
                                                        const uint32_t* __restrict__ layer_off, float4* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * DN_ALBEDO_WAVELENGTHS) return;
    const SceneView s{blob, tex, blob + blob[PT_HDR_CORE_WORDS]};
    const LayerCurves c = layer_curves(s, layer_off[i / DN_ALBEDO_WAVELENGTHS], B.lambda[i % DN_ALBEDO_WAVELENGTHS]);
    table[i] = make_float4(c.c0, c.c1, c.c2, c.c3);
}
// the texture stack of a Lambertian hit: texels from the blob, curve values from the table (material_row: the first table row of the material's layers)
struct TableStack {
    const uint32_t* w; const float* tex; const float4* table; uint32_t ts, row; float u, v;
    __device__ uint32_t layers() const { return w[ts]; }
    __device__ DnTexel texel(uint32_t i) const { return dn_albedo_texel(w, tex, ts + 1u + i * PT_LAYER_WORDS, u, v); }
    __device__ DnLayerCurves curves(uint32_t i, int j) const { const float4 c = table[(row + i) * DN_ALBEDO_WAVELENGTHS + (uint32_t)j]; return DnLayerCurves{c.x, c.y, c.z, c.w}; }
};
__global__ void __launch_bounds__(kLine) k_guide_fold_albedo(uint32_t n, const pt_hit* __restrict__ hits, DnGuideSum* __restrict__ sums, float4* __restrict__ asums, int first,
                                                            const uint32_t* __restrict__ blob, const float* __restrict__ tex, uint32_t material_count,
                                                            const uint32_t* __restrict__ material_row, const float4* __restrict__ table, DnAlbedoBasis B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DnGuideSum g;
    DnAlbedo as;
    if (first) { g.nx = 0.0f; g.ny = 0.0f; g.nz = 0.0f; g.z = 0.0f; g.hits = 0u; as.x = 0.0f; as.y = 0.0f; as.z = 0.0f; }
    else { g = sums[i]; const float4 a4 = asums[i]; as.x = a4.x; as.y = a4.y; as.z = a4.z; }
    const pt_hit h = hits[i];
    dn_guide_add(&g, h.valid, h.t, h.normal[0], h.normal[1], h.normal[2]);
    DnAlbedo a{1.0f, 1.0f, 1.0f};
    if (dn_albedo_has_record(h.valid, h.material, material_count)) {
        const uint32_t mi = PT_MATERIAL_INDEX(h.material), m = blob[PT_HDR_MATERIAL_OFF] + mi * PT_MAT_WORDS;
        if (blob[m + PT_MAT_KIND] == (uint32_t)PT_MATERIAL_LAMBERTIAN)
            a = dn_albedo_lambertian(TableStack{blob, tex, table, blob[m + PT_MAT_TEXSTACK], material_row[mi], h.uv[0], h.uv[1]}, B);
    }
    dn_albedo_add(&as, a);
    sums[i] = g;
    asums[i] = make_float4(as.x, as.y, as.z, 0.0f);
}
__global__ void __launch_bounds__(kLine) k_guide_finish_albedo(uint32_t n, const DnGuideSum* __restrict__ sums, const float4* __restrict__ asums, uint32_t samples,
                                                              float4* __restrict__ guides, float4* __restrict__ albedo) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DnGeo g = dn_guide_finish(sums[i], samples);
    guides[i] = make_float4(g.nx, g.ny, g.nz, g.z);
    const float4 s = asums[i];
    const DnAlbedo a = dn_albedo_finish(DnAlbedo{s.x, s.y, s.z}, samples);
    albedo[i] = make_float4(a.x, a.y, a.z, 0.0f);
}

// ---------------------------------------------------------------------------------------------- filter
struct DnBuffers {
    const float4* color;    // c_i xyz, v_i
    const float4* geo;      // unit normal, depth
    const float* tent;      // the pass's filtered variance
    const uint8_t* flags;   // DN_DEAD | DN_SKY
    const float2* grad;     // depth gradient
};

// the pass's inputs in global memory
struct GlobalSource {
    DnBuffers b; uint32_t width;
    __host__ __device__ uint32_t flags(int x, int y) const { return b.flags[(uint32_t)y * width + (uint32_t)x]; }
    __host__ __device__ DnColor color(int x, int y) const { const float4 c = b.color[(uint32_t)y * width + (uint32_t)x]; return DnColor{c.x, c.y, c.z, c.w}; }
    __host__ __device__ DnGeo geo(int x, int y) const { const float4 g = b.geo[(uint32_t)y * width + (uint32_t)x]; return DnGeo{g.x, g.y, g.z, g.w}; }
    __host__ __device__ float tent(int x, int y) const { return b.tent[(uint32_t)y * width + (uint32_t)x]; }
};

// (ALBEDO false: the lane of pt_denoise_film, as it always was; true: the film demodulated, dn_demodulate)
template <bool ALBEDO>
__device__ __forceinline__ void dn_prepare_lane(const DnParams& P, const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                const float4* __restrict__ guides, const float4* __restrict__ albedo, float4* __restrict__ color, float4* __restrict__ geo,
                                                uint8_t* __restrict__ flags, float2* __restrict__ grad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.width * P.height) return;
    const uint32_t x = i % P.width, y = i / P.width;
    const float4 c = film[i];
    const double2 s = stats[i];
    const float v = dn_variance(counts[i], s.x, s.y);
    const float4 g = guides[i];
    uint32_t sky;
    const DnGeo u = dn_unit(g.x, g.y, g.z, g.w, &sky);
    if (ALBEDO) {
        const float4 a = albedo[i];
        uint32_t dead;
        const DnColor d = dn_demodulate(DnColor{c.x, c.y, c.z, v}, DnAlbedo{a.x, a.y, a.z}, &dead);
        color[i] = make_float4(d.x, d.y, d.z, d.v);
        geo[i] = make_float4(u.nx, u.ny, u.nz, u.z);
        flags[i] = (uint8_t)(dead | sky);
    } else {
        color[i] = make_float4(c.x, c.y, c.z, v);
        geo[i] = make_float4(u.nx, u.ny, u.nz, u.z);
        flags[i] = (uint8_t)(dn_dead(c.x, c.y, c.z, v) | sky);
    }
    // (neighbours' depths: clamped indices, the ends are selected away by dn_gradient)
    const float zl = guides[y * P.width + (x > 0u ? x - 1u : x)].w, zr = guides[y * P.width + (x + 1u < P.width ? x + 1u : x)].w;
    const float zu = guides[(y > 0u ? y - 1u : y) * P.width + x].w, zd = guides[(y + 1u < P.height ? y + 1u : y) * P.width + x].w;
    grad[i] = make_float2(dn_gradient(zl, g.w, zr, x, P.width), dn_gradient(zu, g.w, zd, y, P.height));
}
__global__ void __launch_bounds__(kLine) k_dn_prepare(DnParams P, const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                     const float4* __restrict__ guides, float4* __restrict__ color, float4* __restrict__ geo,
                                                     uint8_t* __restrict__ flags, float2* __restrict__ grad) {
    dn_prepare_lane<false>(P, film, counts, stats, guides, nullptr, color, geo, flags, grad);
}
__global__ void __launch_bounds__(kLine) k_dn_prepare_albedo(DnParams P, const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                            const float4* __restrict__ guides, const float4* __restrict__ albedo, float4* __restrict__ color,
                                                            float4* __restrict__ geo, uint8_t* __restrict__ flags, float2* __restrict__ grad) {
    dn_prepare_lane<true>(P, film, counts, stats, guides, albedo, color, geo, flags, grad);
}

__global__ void __launch_bounds__(kTileW * kTileH) k_dn_tent(DnParams P, DnBuffers b, float* __restrict__ tent) {
    const int x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    if (x >= (int)P.width || y >= (int)P.height) return;
    const GlobalSource src{b, P.width};
    tent[(uint32_t)y * P.width + (uint32_t)x] = dn_tent_pixel(src, P, x, y);
}

__global__ void __launch_bounds__(kTileW * kTileH) k_dn_gather(DnParams P, int step, DnBuffers b, float4* __restrict__ out) {
    const int x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    if (x >= (int)P.width || y >= (int)P.height) return;
    const uint32_t i = (uint32_t)y * P.width + (uint32_t)x;
    const GlobalSource src{b, P.width};
    const float2 g = b.grad[i];
    const DnColor o = dn_gather_pixel(src, P, step, x, y, g.x, g.y);
    out[i] = make_float4(o.x, o.y, o.z, o.v);
}

__global__ void __launch_bounds__(kLine) k_dn_finish(uint32_t n, const float4* __restrict__ color, float4* __restrict__ film, float* __restrict__ variance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = color[i];
    film[i] = make_float4(c.x, c.y, c.z, 0.0f);
    variance[i] = c.w;
}

// (a dead pixel holds its own film values and is not multiplied: the flags say which)
__global__ void __launch_bounds__(kLine) k_dn_finish_albedo(uint32_t n, const float4* __restrict__ color, const float4* __restrict__ albedo, const uint8_t* __restrict__ flags,
                                                           float4* __restrict__ film, float* __restrict__ variance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = color[i], a = albedo[i];
    const DnColor o = dn_remodulate(DnColor{c.x, c.y, c.z, c.w}, DnAlbedo{a.x, a.y, a.z}, flags[i]);
    film[i] = make_float4(o.x, o.y, o.z, 0.0f);
    variance[i] = o.v;
}

// ---------------------------------------------------------------------------------------------- filter, with the bins
// The gather is k_dn_gather's tile (32x8 pixels, one pixel per lane) with the taps kept: the edge-stopping weight of a tap costs about 200 vector instructions
// and depends on the colour and the guides alone, so a lane computes its 25 weights once — the 5x5 loops are fully unrolled, every index is static, and the
// weights and the 25-bit mask of the taps taken stay in registers — writes the colour, and then runs the 25 taps again per chunk of 8 bins: one load, one
// multiply and one add per tap and bin.  Neighbouring lanes read neighbouring pixels of one plane, so every load is a coalesced row segment.  A tap that is
// not taken reads the lane's own pixel and its sum is selected away: no branch in the bin loop, and the loads of a chunk are independent of each other.
// The colour and the bins share one kernel; the alternative — the 25 weights through a 100-byte-per-pixel buffer to a second kernel — was not built: it adds
// 200 bytes of traffic per pixel and pass to save registers this kernel has to spare (DESIGN.md section 14 has the counts).
//
// the pass's inputs in global memory: the film filter's planes and the bins.  A pixel index is a uint32_t as above: normalize_denoise_desc (through
// check_denoise_spectral_args) refuses width x height above 2^31 - 1 before anything is launched; the plane offset b * plane is formed in size_t.
struct SpectralSource {
    const float4* color_; const float4* geo_; const float* tent_; const uint8_t* flags_; const float* bins_; uint32_t width, plane;
    __device__ uint32_t at(int x, int y) const { return (uint32_t)y * width + (uint32_t)x; }
    __device__ uint32_t flags(int x, int y) const { return flags_[at(x, y)]; }
    __device__ DnColor color(int x, int y) const { const float4 c = color_[at(x, y)]; return DnColor{c.x, c.y, c.z, c.w}; }
    __device__ DnGeo geo(int x, int y) const { const float4 g = geo_[at(x, y)]; return DnGeo{g.x, g.y, g.z, g.w}; }
    __device__ float tent(int x, int y) const { return tent_[at(x, y)]; }
    __device__ float bin(uint32_t b, int x, int y) const { return bins_[(size_t)b * plane + at(x, y)]; }
};

// behind k_dn_prepare: flags |= DN_DEAD where a bin of the pixel is not finite
__global__ void __launch_bounds__(kLine) k_dn_spectral_dead(uint32_t n, uint32_t bins, const float* __restrict__ spectral, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t dead = dn_spectral_dead(bins, [&](uint32_t b) { return spectral[(size_t)b * n + i]; });
    if (dead) flags[i] = (uint8_t)(flags[i] | dead);
}

// one a-trous pass: out = c_{i+1}, v_{i+1} (k_dn_gather's, bit for bit) and spectral_out = s_{b,i+1} for every bin.  The outputs must not alias the inputs.
__global__ void __launch_bounds__(kTileW * kTileH, 4) k_dn_gather_spectral(DnParams P, int step, SpectralSource src, const float2* __restrict__ grad, uint32_t bins,
                                                                        float4* __restrict__ out, float* __restrict__ spectral_out) {
    const int x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    if (x >= (int)P.width || y >= (int)P.height) return;
    const uint32_t i = (uint32_t)y * P.width + (uint32_t)x;
    const float2 g = grad[i];
    DnTaps taps;
    const DnColor o = dn_gather_pixel_taps(src, P, step, x, y, g.x, g.y, &taps);
    out[i] = make_float4(o.x, o.y, o.z, o.v);
    float* px = spectral_out + i;
    const uint32_t plane = src.plane;
    dn_gather_pixel_bins(src, step, x, y, taps, bins, [&](uint32_t b, float v) { px[(size_t)b * plane] = v; });
}

// The bins' demodulation, behind k_dn_prepare(_albedo).  One lane per pixel, looping over the planes (neighbouring lanes are neighbouring pixels of one
// plane): raw -> out (which must not be raw), the dead bit into flags, and a pixel that is dead through its bins alone gets k_dn_prepare's colour of a dead
// pixel back (k_dn_prepare_albedo had divided it).  HAS_A false: no per-bin albedo, the bins are copied and tested.
template <bool HAS_A>
__global__ void __launch_bounds__(kLine) k_dn_demodulate_bins(uint32_t n, uint32_t bins, const float* __restrict__ raw, const float* __restrict__ bin_albedo,
                                                             const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                             float* __restrict__ out, float4* __restrict__ color, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    const uint32_t dead = dn_bins_demodulate_pixel(bins, f, [&](uint32_t b) { return raw[(size_t)b * n + i]; },
                                                   [&](uint32_t b) { return HAS_A ? bin_albedo[(size_t)b * n + i] : 1.0f; },
                                                   [&](uint32_t b, float v) { out[(size_t)b * n + i] = v; });
    if (dead && !(f & DN_DEAD)) {
        const float4 c = film[i];
        const double2 s = stats[i];
        const DnColor o = dn_bins_dead_color(c.x, c.y, c.z, counts[i], s.x, s.y);
        color[i] = make_float4(o.x, o.y, o.z, o.v);
        flags[i] = (uint8_t)(f | dead);
    }
}
// after the last pass, over bins x n_pixels values, in place; a dead pixel keeps what the passes copied through: its input bits
__global__ void __launch_bounds__(kLine) k_dn_remodulate_bins(size_t total, uint32_t n, const float* __restrict__ bin_albedo, const uint8_t* __restrict__ flags,
                                                             float* __restrict__ bins) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (flags[i % n] & DN_DEAD) return;
    bins[i] = dn_bin_remodulate(bins[i], bin_albedo[i]);
}

// ---------------------------------------------------------------------------------------------- filter, with the bins as quads
// The resident form's passes (pt_denoise_resident_rules.h): the ping-pong buffers hold quads of four bins per pixel, so the bin loop of a pass issues one
// 16-byte load per tap and quad where k_dn_gather_spectral issues four 4-byte loads.  Neighbouring lanes read neighbouring quads: a wave's load is two rows
// of 512 contiguous bytes.  The pixel index is a uint32_t as above; the quad index q * plane + pixel is formed in size_t.
struct QuadSource {
    const float4* color_; const float4* geo_; const float* tent_; const uint8_t* flags_; const DnQuad* quads_; uint32_t width, plane;
    __device__ uint32_t at(int x, int y) const { return (uint32_t)y * width + (uint32_t)x; }
    __device__ uint32_t flags(int x, int y) const { return flags_[at(x, y)]; }
    __device__ DnColor color(int x, int y) const { const float4 c = color_[at(x, y)]; return DnColor{c.x, c.y, c.z, c.w}; }
    __device__ DnGeo geo(int x, int y) const { const float4 g = geo_[at(x, y)]; return DnGeo{g.x, g.y, g.z, g.w}; }
    __device__ float tent(int x, int y) const { return tent_[at(x, y)]; }
    __device__ DnQuad bin4(uint32_t q, int x, int y) const { return quads_[dn_quad_index(q, plane, at(x, y))]; }
};

// Behind k_dn_prepare(_albedo), in the place of k_dn_demodulate_bins and k_dn_spectral_dead: plane-major raw -> quads (which raw does not alias), divided where
// HAS_A, the dead bit into flags, and a pixel that is dead through its bins alone gets k_dn_prepare's colour of a dead pixel.  One lane per pixel: the reads
// of a plane and the 16-byte stores of a quad plane are both contiguous over a wave.
template <bool HAS_A>
__global__ void __launch_bounds__(kLine) k_dn_bins_to_quads(uint32_t n, uint32_t bins, const float* __restrict__ raw, const float* __restrict__ bin_albedo,
                                                           const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                           DnQuad* __restrict__ quads, float4* __restrict__ color, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    const uint32_t dead = dn_bins_to_quads_pixel(bins, f, [&](uint32_t b) { return raw[(size_t)b * n + i]; },
                                                 [&](uint32_t b) { return HAS_A ? bin_albedo[(size_t)b * n + i] : 1.0f; },
                                                 [&](uint32_t q, DnQuad v) { quads[dn_quad_index(q, n, i)] = v; });
    if (dead && !(f & DN_DEAD)) {
        const float4 c = film[i];
        const double2 s = stats[i];
        const DnColor o = dn_bins_dead_color(c.x, c.y, c.z, counts[i], s.x, s.y);
        color[i] = make_float4(o.x, o.y, o.z, o.v);
        flags[i] = (uint8_t)(f | dead);
    }
}

// one a-trous pass: k_dn_gather_spectral's tile and weight phase, the bins as quads.  The outputs must not alias the inputs.
__global__ void __launch_bounds__(kTileW * kTileH, 4) k_dn_gather_spectral_quad(DnParams P, int step, QuadSource src, const float2* __restrict__ grad, uint32_t quads,
                                                                             float4* __restrict__ out, DnQuad* __restrict__ quads_out) {
    const int x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    if (x >= (int)P.width || y >= (int)P.height) return;
    const uint32_t i = (uint32_t)y * P.width + (uint32_t)x;
    const float2 g = grad[i];
    DnTaps taps;
    const DnColor o = dn_gather_pixel_taps(src, P, step, x, y, g.x, g.y, &taps);
    out[i] = make_float4(o.x, o.y, o.z, o.v);
    DnQuad* px = quads_out + i;
    const uint32_t plane = src.plane;
    dn_gather_pixel_bins4(src, step, x, y, taps, quads, [&](uint32_t q, DnQuad v) { px[(size_t)q * plane] = v; });
}

// after the last pass, in the place of k_dn_remodulate_bins: quads -> plane-major bins, a live pixel's multiplied back where HAS_A
template <bool HAS_A>
__global__ void __launch_bounds__(kLine) k_dn_quads_to_bins(uint32_t n, uint32_t bins, const DnQuad* __restrict__ quads, const float* __restrict__ bin_albedo,
                                                           const uint8_t* __restrict__ flags, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dn_quads_to_bins_pixel<HAS_A>(bins, flags[i], [&](uint32_t q) { return quads[dn_quad_index(q, n, i)]; },
                                  [&](uint32_t b) { return bin_albedo[(size_t)b * n + i]; }, [&](uint32_t b, float v) { out[(size_t)b * n + i] = v; });
}

// ---------------------------------------------------------------------------------------------- filter, with light-group films
// The joint filter over group films (pt_denoise_light_groups_rules.h) in the films' own layout: group-major float4 films, which is the layout dn_quad_index gives
// a quad plane, so nothing is transposed into planes or quads and back.  The gather is k_dn_gather_spectral_quad's text over a GroupSource: its tile and
// weight phase, then one 16-byte load per tap and group in chunks of two groups (dn_gather_pixel_bins4; w rides along as a fourth bin that stays 0).  A text
// of its own that summed three channels, in chunks of four or of two groups, was measured against it and is not kept: no faster at G = 1 and 3 on the whole and
// 4 to 9 % slower at G = 8: the weight phase is most of the kernel, and the fourth channel does not show in its time.
// Neighbouring lanes read neighbouring float4s of one group's film: a wave's load is two rows of 512 contiguous bytes.
struct GroupSource {
    const float4* color_; const float4* geo_; const float* tent_; const uint8_t* flags_; const DnQuad* groups_; uint32_t width, plane;
    __device__ uint32_t at(int x, int y) const { return (uint32_t)y * width + (uint32_t)x; }
    __device__ uint32_t flags(int x, int y) const { return flags_[at(x, y)]; }
    __device__ DnColor color(int x, int y) const { const float4 c = color_[at(x, y)]; return DnColor{c.x, c.y, c.z, c.w}; }
    __device__ DnGeo geo(int x, int y) const { const float4 g = geo_[at(x, y)]; return DnGeo{g.x, g.y, g.z, g.w}; }
    __device__ float tent(int x, int y) const { return tent_[at(x, y)]; }
    __device__ DnQuad bin4(uint32_t g, int x, int y) const { return groups_[dn_quad_index(g, plane, at(x, y))]; }
};

// Behind k_dn_prepare(_albedo): the group films (never written) -> the first ping-pong buffer, divided by the XYZ albedo where HAS_A, the dead bit into flags,
// and a pixel that is dead through its groups alone gets k_dn_prepare's colour of a dead pixel.  One lane per pixel, one 16-byte load and store per group.
template <bool HAS_A>
__global__ void __launch_bounds__(kLine) k_dn_groups_prepare(uint32_t n, uint32_t groups, const DnQuad* __restrict__ raw, const float4* __restrict__ albedo,
                                                            const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                            DnQuad* __restrict__ out, float4* __restrict__ color, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    DnAlbedo a{1.0f, 1.0f, 1.0f};
    if (HAS_A) { const float4 a4 = albedo[i]; a = DnAlbedo{a4.x, a4.y, a4.z}; }
    const uint32_t dead = dn_groups_prepare_pixel<HAS_A>(groups, f, a, [&](uint32_t g) { return raw[dn_quad_index(g, n, i)]; },
                                                         [&](uint32_t g, DnQuad v) { out[dn_quad_index(g, n, i)] = v; });
    if (dead && !(f & DN_DEAD)) {
        const float4 c = film[i];
        const double2 s = stats[i];
        const DnColor o = dn_bins_dead_color(c.x, c.y, c.z, counts[i], s.x, s.y);
        color[i] = make_float4(o.x, o.y, o.z, o.v);
        flags[i] = (uint8_t)(f | dead);
    }
}

// one a-trous pass: k_dn_gather_spectral's tile and weight phase, then the groups.  The outputs must not alias the inputs.
__global__ void __launch_bounds__(kTileW * kTileH, 4) k_dn_gather_groups(DnParams P, int step, GroupSource src, const float2* __restrict__ grad, uint32_t groups,
                                                                      float4* __restrict__ out, DnQuad* __restrict__ groups_out) {
    const int x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
    if (x >= (int)P.width || y >= (int)P.height) return;
    const uint32_t i = (uint32_t)y * P.width + (uint32_t)x;
    const float2 g = grad[i];
    DnTaps taps;
    const DnColor o = dn_gather_pixel_taps(src, P, step, x, y, g.x, g.y, &taps);
    out[i] = make_float4(o.x, o.y, o.z, o.v);
    DnQuad* px = groups_out + i;
    const uint32_t plane = src.plane;
    dn_gather_pixel_bins4(src, step, x, y, taps, groups, [&](uint32_t k, DnQuad v) { px[(size_t)k * plane] = v; });
}

// after the last pass: the ping-pong buffer -> the denoised group films, a live pixel multiplied back where HAS_A, its w 0; a dead one copied through
template <bool HAS_A>
__global__ void __launch_bounds__(kLine) k_dn_groups_finish(uint32_t n, uint32_t groups, const DnQuad* __restrict__ in, const float4* __restrict__ albedo,
                                                           const uint8_t* __restrict__ flags, DnQuad* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    DnAlbedo a{1.0f, 1.0f, 1.0f};
    if (HAS_A) { const float4 a4 = albedo[i]; a = DnAlbedo{a4.x, a4.y, a4.z}; }
    for (uint32_t g = 0; g < groups; ++g) out[dn_quad_index(g, n, i)] = dn_groups_finish_pixel<HAS_A>(f, a, in[dn_quad_index(g, n, i)]);
}

int line_grid(size_t n) { return (int)((n + kLine - 1) / kLine); }

// ---------------------------------------------------------------------------------------------- the filter's driver
struct Dev {
    void* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// host arrays of one call: width x height pixels, the bins and bin_albedo `bins` planes of them
struct DnHost {
    const float* film; const uint32_t* counts; const double* stats; const float* guides;   // required
    const float* albedo; uint32_t bins; const float* spectral; const float* bin_albedo;    // optional: null (bins 0) when absent; bin_albedo only with spectral
    float* out_film; float* out_spectral; float* out_variance;                             // out_spectral with spectral; out_variance may be null
    uint32_t groups; const float* group_films; float* out_group_films;                     // pt_denoise_light_groups: group-major float4 films (groups 0: none)
};

// The filter behind the four host-array entries, which have checked their arguments: `d` is the normalised descriptor.  Three parts: the upload into device
// buffers of this call's own, ptk::dn_run on them (the null stream), and one synchronise before the read-backs.
pt_status dn_filter(const pt_denoise_desc& d, const DnHost& h) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return dfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
    if (d.device >= (uint32_t)ndev) return dfail(PT_ERR_INVALID_ARGUMENT, "device out of range");
#define DN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return dfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    DN_TRY(hipSetDevice((int)d.device));
    const size_t np = (size_t)d.width * d.height, bin_bytes = sizeof(float) * h.bins * np;
    Dev d_film, d_counts, d_stats, d_guides, d_color[2], d_geo, d_tent, d_flags, d_grad, d_var, d_bins[2], d_albedo, d_bin_albedo, d_groups, d_group_buf[2];
    const size_t group_bytes = 16 * np * h.groups;
    DN_TRY(d_film.alloc(16 * np)); DN_TRY(d_counts.alloc(4 * np)); DN_TRY(d_stats.alloc(16 * np)); DN_TRY(d_guides.alloc(16 * np));
    DN_TRY(d_color[0].alloc(16 * np)); DN_TRY(d_color[1].alloc(16 * np)); DN_TRY(d_geo.alloc(16 * np)); DN_TRY(d_tent.alloc(4 * np));
    DN_TRY(d_flags.alloc(np)); DN_TRY(d_grad.alloc(8 * np)); DN_TRY(d_var.alloc(4 * np));
    if (h.spectral) { DN_TRY(d_bins[0].alloc(bin_bytes)); DN_TRY(d_bins[1].alloc(bin_bytes)); }
    DN_TRY(hipMemcpy(d_film.p, h.film, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_counts.p, h.counts, 4 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_stats.p, h.stats, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_guides.p, h.guides, 16 * np, hipMemcpyHostToDevice));
    // the bins are divided, or copied through the dead test of the division, where an albedo is given: from the second ping-pong buffer, which is free until
    // the first pass writes it, into the first.  With no albedo they are tested where they lie.
    const bool demodulate = h.spectral && (h.albedo || h.bin_albedo);
    if (h.spectral) DN_TRY(hipMemcpy(d_bins[demodulate ? 1 : 0].p, h.spectral, bin_bytes, hipMemcpyHostToDevice));
    if (h.albedo) { DN_TRY(d_albedo.alloc(16 * np)); DN_TRY(hipMemcpy(d_albedo.p, h.albedo, 16 * np, hipMemcpyHostToDevice)); }
    if (h.bin_albedo) { DN_TRY(d_bin_albedo.alloc(bin_bytes)); DN_TRY(hipMemcpy(d_bin_albedo.p, h.bin_albedo, bin_bytes, hipMemcpyHostToDevice)); }
    if (h.groups) {   // (the finish writes the denoised films over the uploaded ones: the passes have left them behind by then)
        DN_TRY(d_groups.alloc(group_bytes)); DN_TRY(d_group_buf[0].alloc(group_bytes)); DN_TRY(d_group_buf[1].alloc(group_bytes));
        DN_TRY(hipMemcpy(d_groups.p, h.group_films, group_bytes, hipMemcpyHostToDevice));
    }
    ptk::DnRun r{};
    r.film = d_film.as<float>(); r.counts = d_counts.as<uint32_t>(); r.stats = d_stats.as<double>(); r.guides = d_guides.as<float>();
    r.albedo = d_albedo.as<float>(); r.bins = h.bins; r.spectral = h.spectral ? d_bins[demodulate ? 1 : 0].as<float>() : nullptr; r.bin_albedo = d_bin_albedo.as<float>();
    r.color[0] = d_color[0].as<float>(); r.color[1] = d_color[1].as<float>(); r.geo = d_geo.as<float>(); r.tent = d_tent.as<float>(); r.flags = d_flags.as<uint8_t>();
    r.grad = d_grad.as<float>(); r.bin_buf[0] = d_bins[0].as<float>(); r.bin_buf[1] = d_bins[1].as<float>();
    r.out_film = d_film.as<float>(); r.out_variance = d_var.as<float>();
    r.groups = h.groups; r.group_films = d_groups.as<float>(); r.group_buf[0] = d_group_buf[0].as<float>(); r.group_buf[1] = d_group_buf[1].as<float>();
    r.out_groups = d_groups.as<float>();
    ptk::dn_run(d, &r, nullptr);
    DN_TRY(hipGetLastError());
    DN_TRY(hipDeviceSynchronize());
    DN_TRY(hipMemcpy(h.out_film, r.out_film, 16 * np, hipMemcpyDeviceToHost));
    if (h.spectral) DN_TRY(hipMemcpy(h.out_spectral, r.denoised_bins, bin_bytes, hipMemcpyDeviceToHost));
    if (h.out_variance) DN_TRY(hipMemcpy(h.out_variance, r.out_variance, 4 * np, hipMemcpyDeviceToHost));
    if (h.groups) DN_TRY(hipMemcpy(h.out_group_films, r.out_groups, group_bytes, hipMemcpyDeviceToHost));
#undef DN_TRY
    return PT_OK;
}

}  // namespace

namespace ptk {

void launch_guide_rays(const RenderParams& rp, uint32_t n_pixels, uint32_t sample, float* origins, float* directions) {
    hipLaunchKernelGGL(k_guide_rays, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, rp, n_pixels, sample, origins, directions);
}
void launch_guide_fold(uint32_t n_pixels, const pt_hit* hits, DnGuideSum* sums, bool first) {
    hipLaunchKernelGGL(k_guide_fold, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, hits, sums, first ? 1 : 0);
}
void launch_guide_finish(uint32_t n_pixels, const DnGuideSum* sums, uint32_t samples, float* guides_xyzw) {
    hipLaunchKernelGGL(k_guide_finish, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, sums, samples, reinterpret_cast<float4*>(guides_xyzw));
}

void launch_albedo_tables(const uint32_t* blob, const float* tex, const DnAlbedoBasis& basis, uint32_t rows, const uint32_t* layer_off, float* table) {
    if (rows == 0) return;
    hipLaunchKernelGGL(k_albedo_tables, dim3(line_grid((size_t)rows * DN_ALBEDO_WAVELENGTHS)), dim3(kLine), 0, 0, blob, tex, basis, rows, layer_off, reinterpret_cast<float4*>(table));
}
void launch_guide_fold_albedo(uint32_t n_pixels, const pt_hit* hits, DnGuideSum* sums, float* albedo_sums, bool first, const uint32_t* blob, const float* tex,
                              uint32_t material_count, const uint32_t* material_row, const float* table, const DnAlbedoBasis& basis) {
    hipLaunchKernelGGL(k_guide_fold_albedo, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, hits, sums, reinterpret_cast<float4*>(albedo_sums), first ? 1 : 0, blob, tex,
                       material_count, material_row, reinterpret_cast<const float4*>(table), basis);
}
void launch_guide_finish_albedo(uint32_t n_pixels, const DnGuideSum* sums, const float* albedo_sums, uint32_t samples, float* guides_xyzw, float* albedo_xyzw) {
    hipLaunchKernelGGL(k_guide_finish_albedo, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, sums, reinterpret_cast<const float4*>(albedo_sums), samples,
                       reinterpret_cast<float4*>(guides_xyzw), reinterpret_cast<float4*>(albedo_xyzw));
}
void albedo_basis(float wavelength_lo, float wavelength_hi, DnAlbedoBasis* basis) {
    dn_albedo_basis(wavelength_lo, wavelength_hi, [](float angstrom, float* x, float* y, float* z) { xyz_bar(angstrom, x, y, z); }, basis);
}


// The run of the filter on device pointers (pt_denoise_resident_launch.h).  The launches are, kernel for kernel and in order, what the host-array entries have
// always launched; `quads` swaps the three kernels that touch the bins for their quad forms.  `groups` (light-group films, never beside bins) adds the group
// prepare behind the film's, takes the group gather in every pass and adds the group finish behind the film's; with no groups nothing of that is launched.
void dn_run(const pt_denoise_desc& d, DnRun* run, hipStream_t stream) {
    const DnRun& r = *run;
    const size_t np = (size_t)d.width * d.height;
    const uint32_t n = (uint32_t)np;
    DnParams P;
    P.width = d.width; P.height = d.height; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    const float4 *film = reinterpret_cast<const float4*>(r.film), *guides = reinterpret_cast<const float4*>(r.guides), *albedo = reinterpret_cast<const float4*>(r.albedo);
    const double2* stats = reinterpret_cast<const double2*>(r.stats);
    float4* color[2] = {reinterpret_cast<float4*>(r.color[0]), reinterpret_cast<float4*>(r.color[1])};
    float4* geo = reinterpret_cast<float4*>(r.geo);
    float2* grad = reinterpret_cast<float2*>(r.grad);
    const dim3 line(line_grid(np)), line_block(kLine);
    if (r.albedo) hipLaunchKernelGGL(k_dn_prepare_albedo, line, line_block, 0, stream, P, film, r.counts, stats, guides, albedo, color[0], geo, r.flags, grad);
    else hipLaunchKernelGGL(k_dn_prepare, line, line_block, 0, stream, P, film, r.counts, stats, guides, color[0], geo, r.flags, grad);
    if (r.spectral && r.quads) {
        const auto k = r.bin_albedo ? k_dn_bins_to_quads<true> : k_dn_bins_to_quads<false>;
        hipLaunchKernelGGL(k, line, line_block, 0, stream, n, r.bins, r.spectral, r.bin_albedo, film, r.counts, stats, reinterpret_cast<DnQuad*>(r.bin_buf[0]), color[0], r.flags);
    } else if (r.spectral && r.spectral != r.bin_buf[0]) {
        const auto k = r.bin_albedo ? k_dn_demodulate_bins<true> : k_dn_demodulate_bins<false>;
        hipLaunchKernelGGL(k, line, line_block, 0, stream, n, r.bins, r.spectral, r.bin_albedo, film, r.counts, stats, r.bin_buf[0], color[0], r.flags);
    } else if (r.spectral) {
        hipLaunchKernelGGL(k_dn_spectral_dead, line, line_block, 0, stream, n, r.bins, r.bin_buf[0], r.flags);
    }
    DnQuad* group_buf[2] = {reinterpret_cast<DnQuad*>(r.group_buf[0]), reinterpret_cast<DnQuad*>(r.group_buf[1])};
    if (r.groups) {
        const auto k = r.albedo ? k_dn_groups_prepare<true> : k_dn_groups_prepare<false>;
        hipLaunchKernelGGL(k, line, line_block, 0, stream, n, r.groups, reinterpret_cast<const DnQuad*>(r.group_films), albedo, film, r.counts, stats, group_buf[0], color[0], r.flags);
    }
    const dim3 grid((d.width + kTileW - 1) / kTileW, (d.height + kTileH - 1) / kTileH), block(kTileW, kTileH);
    int cur = 0;
    for (uint32_t i = 0; i < d.iterations; ++i) {
        const int step = 1 << i;
        const DnBuffers b{color[cur], geo, r.tent, r.flags, grad};
        float4* out = color[cur ^ 1];
        hipLaunchKernelGGL(k_dn_tent, grid, block, 0, stream, P, b, r.tent);
        if (r.groups) {
            const GroupSource src{b.color, b.geo, b.tent, b.flags, group_buf[cur], d.width, n};
            hipLaunchKernelGGL(k_dn_gather_groups, grid, block, 0, stream, P, step, src, b.grad, r.groups, out, group_buf[cur ^ 1]);
        } else if (r.spectral && r.quads) {
            const QuadSource src{b.color, b.geo, b.tent, b.flags, reinterpret_cast<const DnQuad*>(r.bin_buf[cur]), d.width, n};
            hipLaunchKernelGGL(k_dn_gather_spectral_quad, grid, block, 0, stream, P, step, src, b.grad, dn_quad_count(r.bins), out, reinterpret_cast<DnQuad*>(r.bin_buf[cur ^ 1]));
        } else if (r.spectral) {
            const SpectralSource src{b.color, b.geo, b.tent, b.flags, r.bin_buf[cur], d.width, n};
            hipLaunchKernelGGL(k_dn_gather_spectral, grid, block, 0, stream, P, step, src, b.grad, r.bins, out, r.bin_buf[cur ^ 1]);
        } else {
            hipLaunchKernelGGL(k_dn_gather, grid, block, 0, stream, P, step, b, out);
        }
        cur ^= 1;
    }
    if (r.albedo) hipLaunchKernelGGL(k_dn_finish_albedo, line, line_block, 0, stream, n, color[cur], albedo, r.flags, reinterpret_cast<float4*>(r.out_film), r.out_variance);
    else hipLaunchKernelGGL(k_dn_finish, line, line_block, 0, stream, n, color[cur], reinterpret_cast<float4*>(r.out_film), r.out_variance);
    if (r.groups) {
        const auto k = r.albedo ? k_dn_groups_finish<true> : k_dn_groups_finish<false>;
        hipLaunchKernelGGL(k, line, line_block, 0, stream, n, r.groups, group_buf[cur], albedo, r.flags, reinterpret_cast<DnQuad*>(r.out_groups));
    }
    run->denoised_bins = nullptr;
    if (r.spectral && r.quads) {
        const auto k = r.bin_albedo ? k_dn_quads_to_bins<true> : k_dn_quads_to_bins<false>;
        hipLaunchKernelGGL(k, line, line_block, 0, stream, n, r.bins, reinterpret_cast<const DnQuad*>(r.bin_buf[cur]), r.bin_albedo, r.flags, r.out_bins);
        run->denoised_bins = r.out_bins;
    } else if (r.spectral) {
        if (r.bin_albedo) {
            const size_t total = (size_t)r.bins * np;
            hipLaunchKernelGGL(k_dn_remodulate_bins, dim3(line_grid(total)), line_block, 0, stream, total, n, r.bin_albedo, r.flags, r.bin_buf[cur]);
        }
        run->denoised_bins = r.bin_buf[cur];
    }
}

}  // namespace ptk

extern "C" pt_status pt_albedo_basis(const pt_render_desc* desc, float* lambda, float* xyz) {
    std::string err;
    const pt_status st = pth::check_albedo_basis_args(desc, lambda, xyz, &err);
    if (st != PT_OK) return dfail(st, err);
    DnAlbedoBasis B;
    ptk::albedo_basis(desc->wavelength_lo, desc->wavelength_hi, &B);
    memcpy(lambda, B.lambda, sizeof(B.lambda));
    memcpy(xyz, B.w, sizeof(B.w));
    return PT_OK;
}

extern "C" pt_status pt_denoise_film(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                     float* out_film, float* out_variance) {
    return pt_denoise_film_albedo(desc, film, sample_counts, stats, guides, nullptr, out_film, out_variance);
}

extern "C" pt_status pt_denoise_film_albedo(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                            const float* albedo, float* out_film, float* out_variance) {
    pt_denoise_desc d;
    std::string err;
    pt_status st = pth::normalize_denoise_desc(desc, film, sample_counts, stats, guides, out_film, &d, &err);
    if (st == PT_OK) st = pth::check_denoise_inputs(d, sample_counts, guides, &err);
    if (st == PT_OK && albedo) st = pth::check_denoise_albedo(d, albedo, &err);
    if (st != PT_OK) return dfail(st, err);
    return dn_filter(d, DnHost{film, sample_counts, stats, guides, albedo, 0u, nullptr, nullptr, out_film, nullptr, out_variance});
}

extern "C" pt_status pt_denoise_spectral(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                         const float* spectral, float* out_film, float* out_spectral, float* out_variance) {
    pt_denoise_desc d;
    std::string err;
    const pt_status st = pth::check_denoise_spectral_args(desc, bins, film, sample_counts, stats, guides, spectral, out_film, out_spectral, &d, &err);
    if (st != PT_OK) return dfail(st, err);
    return dn_filter(d, DnHost{film, sample_counts, stats, guides, nullptr, bins, spectral, nullptr, out_film, out_spectral, out_variance});
}

extern "C" pt_status pt_denoise_spectral_albedo(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats,
                                                const float* guides, const float* albedo, const float* spectral, const float* bin_albedo, float* out_film,
                                                float* out_spectral, float* out_variance) {
    pt_denoise_desc d;
    std::string err;
    const pt_status st = pth::check_denoise_spectral_albedo_args(desc, bins, film, sample_counts, stats, guides, albedo, spectral, bin_albedo, out_film, out_spectral, &d, &err);
    if (st != PT_OK) return dfail(st, err);
    return dn_filter(d, DnHost{film, sample_counts, stats, guides, albedo, bins, spectral, bin_albedo, out_film, out_spectral, out_variance});
}

extern "C" pt_status pt_denoise_light_groups(const pt_denoise_desc* desc, uint32_t group_count, const float* film, const uint32_t* sample_counts, const double* stats,
                                             const float* guides, const float* albedo, const float* group_films, float* out_film, float* out_variance,
                                             float* out_group_films) {
    pt_denoise_desc d;
    std::string err;
    const pt_status st = pth::check_denoise_light_groups_args(desc, group_count, film, sample_counts, stats, guides, albedo, group_films, out_film, out_group_films, &d, &err);
    if (st != PT_OK) return dfail(st, err);
    return dn_filter(d, DnHost{film, sample_counts, stats, guides, albedo, 0u, nullptr, nullptr, out_film, nullptr, out_variance, group_count, group_films, out_group_films});
}
