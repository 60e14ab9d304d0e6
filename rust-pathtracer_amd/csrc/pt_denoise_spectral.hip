// pt_denoise_spectral.hip — the joint filter of the film and its wavelength bins (pt_denoise_spectral of include/pt_spectral.h) on
// gfx950: the kernel that marks a pixel with a non-finite bin dead, the gather of one a-trous pass over the colour and every bin plane, and the entry itself.
// Prepare, the variance tent and the finish are pt_denoise.hip's kernels, unchanged.  Every per-pixel rule is pt_denoise_spectral_rules.h's, the text the
// host emulation compiles, so the outputs agree with it bit for bit.
//
// The gather is k_dn_gather's tile (32x8 pixels, one pixel per lane) with the taps kept: the edge-stopping weight of a tap costs about 200 vector instructions
// and depends on the colour and the guides alone, so a lane computes its 25 weights once — the 5x5 loops are fully unrolled, every index is static, and the
// weights and the 25-bit mask of the taps taken stay in registers — writes the colour, and then runs the 25 taps again per chunk of 8 bins: one load, one
// multiply and one add per tap and bin.  Neighbouring lanes read neighbouring pixels of one plane, so every load is a coalesced row segment.  A tap that is
// not taken reads the lane's own pixel and its sum is selected away: no branch in the bin loop, and the loads of a chunk are independent of each other.
// The colour and the bins share one kernel; the alternative — the 25 weights through a 100-byte-per-pixel buffer to a second kernel — was not built: it adds
// 200 bytes of traffic per pixel and pass to save registers this kernel has to spare (DESIGN.md section 14 has the counts).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pt_spectral.h"
#include "pt_denoise_launch.h"
#include "pt_denoise_spectral_launch.h"
#include "pt_denoise_spectral_rules.h"
#include "pt_error.h"
#include "pt_plan.h"

using namespace ptd;

namespace {

constexpr int kLine = 256;              // the one-dimensional kernel
constexpr int kTileW = 32, kTileH = 8;  // the gather, as k_dn_gather

pt_status dfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }

// the pass's inputs in global memory: pt_denoise.hip's planes and the bins.  A pixel index is a uint32_t as in pt_denoise.hip: normalize_denoise_desc (through
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

__global__ void __launch_bounds__(kLine) k_dn_spectral_dead(uint32_t n, uint32_t bins, const float* __restrict__ spectral, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t dead = dn_spectral_dead(bins, [&](uint32_t b) { return spectral[(size_t)b * n + i]; });
    if (dead) flags[i] = (uint8_t)(flags[i] | dead);
}

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

struct Dev {
    void* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

namespace ptk {

void launch_dn_spectral_dead(uint32_t n_pixels, uint32_t bins, const float* spectral, uint8_t* flags) {
    hipLaunchKernelGGL(k_dn_spectral_dead, dim3((n_pixels + kLine - 1) / kLine), dim3(kLine), 0, 0, n_pixels, bins, spectral, flags);
}
void launch_dn_gather_spectral(const DnParams& P, int step, const float* color, const float* geo, const float* tent, const uint8_t* flags, const float* grad, uint32_t bins,
                               const float* spectral, float* color_out, float* spectral_out) {
    const SpectralSource src{reinterpret_cast<const float4*>(color), reinterpret_cast<const float4*>(geo), tent, flags, spectral, P.width, P.width * P.height};
    hipLaunchKernelGGL(k_dn_gather_spectral, dim3((P.width + kTileW - 1) / kTileW, (P.height + kTileH - 1) / kTileH), dim3(kTileW, kTileH), 0, 0, P, step, src,
                       reinterpret_cast<const float2*>(grad), bins, reinterpret_cast<float4*>(color_out), spectral_out);
}

}  // namespace ptk

extern "C" pt_status pt_denoise_spectral(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats, const float* guides,
                                         const float* spectral, float* out_film, float* out_spectral, float* out_variance) {
    pt_denoise_desc d;
    std::string err;
    const pt_status st = pth::check_denoise_spectral_args(desc, bins, film, sample_counts, stats, guides, spectral, out_film, out_spectral, &d, &err);
    if (st != PT_OK) return dfail(st, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return dfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
    if (d.device >= (uint32_t)ndev) return dfail(PT_ERR_INVALID_ARGUMENT, "device out of range");
#define DN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return dfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    DN_TRY(hipSetDevice((int)d.device));
    const size_t np = (size_t)d.width * d.height, bin_bytes = sizeof(float) * bins * np;
    Dev d_film, d_counts, d_stats, d_guides, d_color[2], d_geo, d_tent, d_flags, d_grad, d_var, d_bins[2];
    DN_TRY(d_film.alloc(16 * np)); DN_TRY(d_counts.alloc(4 * np)); DN_TRY(d_stats.alloc(16 * np)); DN_TRY(d_guides.alloc(16 * np));
    DN_TRY(d_color[0].alloc(16 * np)); DN_TRY(d_color[1].alloc(16 * np)); DN_TRY(d_geo.alloc(16 * np)); DN_TRY(d_tent.alloc(4 * np));
    DN_TRY(d_flags.alloc(np)); DN_TRY(d_grad.alloc(8 * np)); DN_TRY(d_var.alloc(4 * np));
    DN_TRY(d_bins[0].alloc(bin_bytes)); DN_TRY(d_bins[1].alloc(bin_bytes));
    DN_TRY(hipMemcpy(d_film.p, film, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_counts.p, sample_counts, 4 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_stats.p, stats, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_guides.p, guides, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_bins[0].p, spectral, bin_bytes, hipMemcpyHostToDevice));
    DnParams P;
    P.width = d.width; P.height = d.height; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    ptk::launch_dn_prepare(P, d_film.as<float>(), d_counts.as<uint32_t>(), d_stats.as<double>(), d_guides.as<float>(), d_color[0].as<float>(), d_geo.as<float>(),
                           d_flags.as<uint8_t>(), d_grad.as<float>());
    ptk::launch_dn_spectral_dead((uint32_t)np, bins, d_bins[0].as<float>(), d_flags.as<uint8_t>());
    int cur = 0;
    for (uint32_t i = 0; i < d.iterations; ++i) {
        ptk::launch_dn_tent(P, d_color[cur].as<float>(), d_geo.as<float>(), d_flags.as<uint8_t>(), d_tent.as<float>());
        ptk::launch_dn_gather_spectral(P, 1 << i, d_color[cur].as<float>(), d_geo.as<float>(), d_tent.as<float>(), d_flags.as<uint8_t>(), d_grad.as<float>(), bins,
                                       d_bins[cur].as<float>(), d_color[cur ^ 1].as<float>(), d_bins[cur ^ 1].as<float>());
        cur ^= 1;
    }
    ptk::launch_dn_finish((uint32_t)np, d_color[cur].as<float>(), d_film.as<float>(), d_var.as<float>());
    DN_TRY(hipGetLastError());
    DN_TRY(hipDeviceSynchronize());
    DN_TRY(hipMemcpy(out_film, d_film.p, 16 * np, hipMemcpyDeviceToHost));
    DN_TRY(hipMemcpy(out_spectral, d_bins[cur].p, bin_bytes, hipMemcpyDeviceToHost));
    if (out_variance) DN_TRY(hipMemcpy(out_variance, d_var.p, 4 * np, hipMemcpyDeviceToHost));
#undef DN_TRY
    return PT_OK;
}
