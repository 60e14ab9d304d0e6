// pt_denoise.hip — the film denoiser of include/pt_denoise.h on gfx950: the kernels of the guide pass (camera rays of one
// sample index for every pixel, the fold of the closest-hit probe's records, the final division) and of the filter (prepare, and per a-trous pass
// the 3x3 variance tent and the 25-tap gather over ping-pong buffers), and pt_denoise_film itself.  Every per-pixel rule is pt_denoise_rules.h's,
// the text the host emulation compiles, so the outputs agree with it bit for bit.
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

__global__ void __launch_bounds__(kLine) k_dn_prepare(DnParams P, const float4* __restrict__ film, const uint32_t* __restrict__ counts, const double2* __restrict__ stats,
                                                     const float4* __restrict__ guides, float4* __restrict__ color, float4* __restrict__ geo,
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
    color[i] = make_float4(c.x, c.y, c.z, v);
    geo[i] = make_float4(u.nx, u.ny, u.nz, u.z);
    flags[i] = (uint8_t)(dn_dead(c.x, c.y, c.z, v) | sky);
    // (neighbours' depths: clamped indices, the ends are selected away by dn_gradient)
    const float zl = guides[y * P.width + (x > 0u ? x - 1u : x)].w, zr = guides[y * P.width + (x + 1u < P.width ? x + 1u : x)].w;
    const float zu = guides[(y > 0u ? y - 1u : y) * P.width + x].w, zd = guides[(y + 1u < P.height ? y + 1u : y) * P.width + x].w;
    grad[i] = make_float2(dn_gradient(zl, g.w, zr, x, P.width), dn_gradient(zu, g.w, zd, y, P.height));
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

}  // namespace ptk

extern "C" pt_status pt_denoise_film(const pt_denoise_desc* desc, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                     float* out_film, float* out_variance) {
    pt_denoise_desc d;
    std::string err;
    pt_status st = pth::normalize_denoise_desc(desc, film, sample_counts, stats, guides, out_film, &d, &err);
    if (st == PT_OK) st = pth::check_denoise_inputs(d, sample_counts, guides, &err);
    if (st != PT_OK) return dfail(st, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return dfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
    if (d.device >= (uint32_t)ndev) return dfail(PT_ERR_INVALID_ARGUMENT, "device out of range");
#define DN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return dfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    DN_TRY(hipSetDevice((int)d.device));
    const size_t np = (size_t)d.width * d.height;
    Dev d_film, d_counts, d_stats, d_guides, d_color[2], d_geo, d_tent, d_flags, d_grad, d_var;
    DN_TRY(d_film.alloc(16 * np)); DN_TRY(d_counts.alloc(4 * np)); DN_TRY(d_stats.alloc(16 * np)); DN_TRY(d_guides.alloc(16 * np));
    DN_TRY(d_color[0].alloc(16 * np)); DN_TRY(d_color[1].alloc(16 * np)); DN_TRY(d_geo.alloc(16 * np)); DN_TRY(d_tent.alloc(4 * np));
    DN_TRY(d_flags.alloc(np)); DN_TRY(d_grad.alloc(8 * np)); DN_TRY(d_var.alloc(4 * np));
    DN_TRY(hipMemcpy(d_film.p, film, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_counts.p, sample_counts, 4 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_stats.p, stats, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_guides.p, guides, 16 * np, hipMemcpyHostToDevice));
    DnParams P;
    P.width = d.width; P.height = d.height; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
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
    hipLaunchKernelGGL(k_dn_finish, dim3(line_grid(np)), dim3(kLine), 0, 0, (uint32_t)np, d_color[cur].as<float4>(), d_film.as<float4>(), d_var.as<float>());
    DN_TRY(hipGetLastError());
    DN_TRY(hipDeviceSynchronize());
    DN_TRY(hipMemcpy(out_film, d_film.p, 16 * np, hipMemcpyDeviceToHost));
    if (out_variance) DN_TRY(hipMemcpy(out_variance, d_var.p, 4 * np, hipMemcpyDeviceToHost));
#undef DN_TRY
    return PT_OK;
}
