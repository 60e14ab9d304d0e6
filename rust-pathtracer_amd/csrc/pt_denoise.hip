// pt_denoise.hip — the film denoiser of include/pt_denoise.h on gfx950: the kernels of the guide pass (camera rays of one
// sample index for every pixel, the fold of the closest-hit probe's records, the final division) and of the filter (prepare, and per a-trous pass
// the 3x3 variance tent and the 25-tap gather over ping-pong buffers), of the albedo guide (curve tables, the fold and the division with a second
// sum), and pt_denoise_film(_albedo) itself.  Every per-pixel rule is pt_denoise_rules.h's, the text the host emulation compiles, so the outputs
// agree with it bit for bit.
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
#include "pt_denoise_launch.h"
#include "pt_denoise_rules.h"
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

struct Dev {
    void* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

int line_grid(size_t n) { return (int)((n + kLine - 1) / kLine); }

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


// the filter's kernels for pt_denoise_spectral and pt_denoise_spectral_albedo (pt_denoise_spectral.hip, pt_denoise_spectral_albedo.hip), unchanged
void launch_dn_prepare(const DnParams& P, const float* film, const uint32_t* counts, const double* stats, const float* guides, float* color, float* geo, uint8_t* flags,
                       float* grad) {
    hipLaunchKernelGGL(k_dn_prepare, dim3(line_grid((size_t)P.width * P.height)), dim3(kLine), 0, 0, P, reinterpret_cast<const float4*>(film), counts,
                       reinterpret_cast<const double2*>(stats), reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(color), reinterpret_cast<float4*>(geo), flags,
                       reinterpret_cast<float2*>(grad));
}
void launch_dn_prepare_albedo(const DnParams& P, const float* film, const uint32_t* counts, const double* stats, const float* guides, const float* albedo, float* color,
                              float* geo, uint8_t* flags, float* grad) {
    hipLaunchKernelGGL(k_dn_prepare_albedo, dim3(line_grid((size_t)P.width * P.height)), dim3(kLine), 0, 0, P, reinterpret_cast<const float4*>(film), counts,
                       reinterpret_cast<const double2*>(stats), reinterpret_cast<const float4*>(guides), reinterpret_cast<const float4*>(albedo),
                       reinterpret_cast<float4*>(color), reinterpret_cast<float4*>(geo), flags, reinterpret_cast<float2*>(grad));
}
void launch_dn_tent(const DnParams& P, const float* color, const float* geo, const uint8_t* flags, float* tent) {
    const DnBuffers b{reinterpret_cast<const float4*>(color), reinterpret_cast<const float4*>(geo), tent, flags, nullptr};
    hipLaunchKernelGGL(k_dn_tent, dim3((P.width + kTileW - 1) / kTileW, (P.height + kTileH - 1) / kTileH), dim3(kTileW, kTileH), 0, 0, P, b, tent);
}
void launch_dn_finish(uint32_t n_pixels, const float* color, float* film, float* variance) {
    hipLaunchKernelGGL(k_dn_finish, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, reinterpret_cast<const float4*>(color), reinterpret_cast<float4*>(film), variance);
}
void launch_dn_finish_albedo(uint32_t n_pixels, const float* color, const float* albedo, const uint8_t* flags, float* film, float* variance) {
    hipLaunchKernelGGL(k_dn_finish_albedo, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, reinterpret_cast<const float4*>(color),
                       reinterpret_cast<const float4*>(albedo), flags, reinterpret_cast<float4*>(film), variance);
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return dfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
    if (d.device >= (uint32_t)ndev) return dfail(PT_ERR_INVALID_ARGUMENT, "device out of range");
#define DN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return dfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    DN_TRY(hipSetDevice((int)d.device));
    const size_t np = (size_t)d.width * d.height;
    Dev d_film, d_counts, d_stats, d_guides, d_color[2], d_geo, d_tent, d_flags, d_grad, d_var, d_albedo;
    DN_TRY(d_film.alloc(16 * np)); DN_TRY(d_counts.alloc(4 * np)); DN_TRY(d_stats.alloc(16 * np)); DN_TRY(d_guides.alloc(16 * np));
    DN_TRY(d_color[0].alloc(16 * np)); DN_TRY(d_color[1].alloc(16 * np)); DN_TRY(d_geo.alloc(16 * np)); DN_TRY(d_tent.alloc(4 * np));
    DN_TRY(d_flags.alloc(np)); DN_TRY(d_grad.alloc(8 * np)); DN_TRY(d_var.alloc(4 * np));
    DN_TRY(hipMemcpy(d_film.p, film, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_counts.p, sample_counts, 4 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_stats.p, stats, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_guides.p, guides, 16 * np, hipMemcpyHostToDevice));
    if (albedo) { DN_TRY(d_albedo.alloc(16 * np)); DN_TRY(hipMemcpy(d_albedo.p, albedo, 16 * np, hipMemcpyHostToDevice)); }
    DnParams P;
    P.width = d.width; P.height = d.height; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    if (albedo)
        hipLaunchKernelGGL(k_dn_prepare_albedo, dim3(line_grid(np)), dim3(kLine), 0, 0, P, d_film.as<float4>(), d_counts.as<uint32_t>(), d_stats.as<double2>(), d_guides.as<float4>(),
                           d_albedo.as<float4>(), d_color[0].as<float4>(), d_geo.as<float4>(), d_flags.as<uint8_t>(), d_grad.as<float2>());
    else
        hipLaunchKernelGGL(k_dn_prepare, dim3(line_grid(np)), dim3(kLine), 0, 0, P, d_film.as<float4>(), d_counts.as<uint32_t>(), d_stats.as<double2>(), d_guides.as<float4>(),
                           d_color[0].as<float4>(), d_geo.as<float4>(), d_flags.as<uint8_t>(), d_grad.as<float2>());
    const dim3 grid((d.width + kTileW - 1) / kTileW, (d.height + kTileH - 1) / kTileH), block(kTileW, kTileH);
    int cur = 0;
    for (uint32_t i = 0; i < d.iterations; ++i) {
        const int step = 1 << i;
        const DnBuffers b{d_color[cur].as<float4>(), d_geo.as<float4>(), d_tent.as<float>(), d_flags.as<uint8_t>(), d_grad.as<float2>()};
        float4* out = d_color[cur ^ 1].as<float4>();
        hipLaunchKernelGGL(k_dn_tent, grid, block, 0, 0, P, b, d_tent.as<float>());
        hipLaunchKernelGGL(k_dn_gather, grid, block, 0, 0, P, step, b, out);
        cur ^= 1;
    }
    if (albedo)
        hipLaunchKernelGGL(k_dn_finish_albedo, dim3(line_grid(np)), dim3(kLine), 0, 0, (uint32_t)np, d_color[cur].as<float4>(), d_albedo.as<float4>(), d_flags.as<uint8_t>(),
                           d_film.as<float4>(), d_var.as<float>());
    else
        hipLaunchKernelGGL(k_dn_finish, dim3(line_grid(np)), dim3(kLine), 0, 0, (uint32_t)np, d_color[cur].as<float4>(), d_film.as<float4>(), d_var.as<float>());
    DN_TRY(hipGetLastError());
    DN_TRY(hipDeviceSynchronize());
    DN_TRY(hipMemcpy(out_film, d_film.p, 16 * np, hipMemcpyDeviceToHost));
    if (out_variance) DN_TRY(hipMemcpy(out_variance, d_var.p, 4 * np, hipMemcpyDeviceToHost));
#undef DN_TRY
    return PT_OK;
}
