// pt_denoise_spectral_albedo.hip — the per-bin albedo guide's kernels and the joint filter that demodulates the bins by it (pt_render_guides_bin_albedo and
// pt_denoise_spectral_albedo of include/pt_spectral.h, DESIGN.md section 14, "Demodulating the bins") on gfx950.
//
// The guide: k_bin_albedo_tables is k_albedo_tables over rows x bins with the bins' centre wavelengths; k_guide_fold_bins folds one guide sample's first-hit
// records into the bin-major sums (launched behind k_guide_fold_albedo, which keeps the guide sum and the XYZ albedo sum as it always did; the chain folds the
// same way inside k_chain_step); k_bin_albedo_finish divides by K.  The filter: k_dn_demodulate_bins, behind k_dn_prepare(_albedo), divides the bins and makes
// the dead test; the passes are pt_denoise_spectral's kernels, launched unchanged; k_dn_remodulate_bins multiplies the live pixels' bins back after the last
// pass.  The two filter kernels stream planes: neighbouring lanes are neighbouring pixels of one plane.  Every per-pixel rule is
// pt_denoise_spectral_albedo_rules.h's, the text the host emulation compiles, so the outputs agree with it bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pt_spectral.h"
#include "pt_bin_albedo_device.h"
#include "pt_denoise_launch.h"
#include "pt_denoise_spectral_albedo_launch.h"
#include "pt_denoise_spectral_albedo_rules.h"
#include "pt_denoise_spectral_launch.h"
#include "pt_device.h"
#include "pt_error.h"
#include "pt_plan.h"

using namespace ptd;

namespace {

constexpr int kLine = 256;

pt_status dfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }
inline uint32_t line_grid(size_t n) { return (uint32_t)((n + kLine - 1) / kLine); }

// ---------------------------------------------------------------------------------------------- guide
// one lane per (texture layer of a Lambertian material, bin): the layer's curves at the bin's centre wavelength
__global__ void __launch_bounds__(kLine) k_bin_albedo_tables(const uint32_t* __restrict__ blob, const float* __restrict__ tex, float lo, float width, uint32_t bins, uint32_t rows,
                                                            const uint32_t* __restrict__ layer_off, float4* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * bins) return;   // (rows x bins: at most the scene's layers x 64)
    const SceneView s{blob, tex, blob + blob[PT_HDR_CORE_WORDS]};
    const LayerCurves c = layer_curves(s, layer_off[i / bins], dn_bin_centre(lo, width, i % bins));
    table[i] = make_float4(c.c0, c.c1, c.c2, c.c3);
}
__global__ void __launch_bounds__(kLine) k_guide_fold_bins(uint32_t n, const pt_hit* __restrict__ hits, ptk::BinAlbedoFold F, const uint32_t* __restrict__ blob,
                                                          const float* __restrict__ tex, uint32_t material_count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ptk::bin_albedo_fold_hit(F, i, hits[i], blob, tex, material_count);
}
// over bins x n_pixels values; bin_albedo may be sums (a lane reads and writes its own value)
__global__ void __launch_bounds__(kLine) k_bin_albedo_finish(size_t n, const float* sums, uint32_t samples, float* bin_albedo) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bin_albedo[i] = dn_bin_albedo_finish(sums[i], samples);
}

// ---------------------------------------------------------------------------------------------- filter
// One lane per pixel, looping over the planes: raw -> bins (which must not be raw), the dead bit into flags, and a pixel that is dead through its bins alone
// gets k_dn_prepare's colour of a dead pixel back (k_dn_prepare_albedo had divided it).  HAS_A false: no per-bin albedo, the bins are copied and tested.
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
// over bins x n_pixels values, in place; a dead pixel keeps what the passes copied through: its input bits
__global__ void __launch_bounds__(kLine) k_dn_remodulate_bins(size_t total, uint32_t n, const float* __restrict__ bin_albedo, const uint8_t* __restrict__ flags,
                                                             float* __restrict__ bins) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (flags[i % n] & DN_DEAD) return;
    bins[i] = dn_bin_remodulate(bins[i], bin_albedo[i]);
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

void launch_bin_albedo_tables(const uint32_t* blob, const float* tex, float wavelength_lo, float bin_width, uint32_t bins, uint32_t rows, const uint32_t* layer_off, float* table) {
    if (rows == 0) return;
    hipLaunchKernelGGL(k_bin_albedo_tables, dim3(line_grid((size_t)rows * bins)), dim3(kLine), 0, 0, blob, tex, wavelength_lo, bin_width, bins, rows, layer_off,
                       reinterpret_cast<float4*>(table));
}
void launch_guide_fold_bins(uint32_t n_pixels, const pt_hit* hits, const BinAlbedoFold& fold, const uint32_t* blob, const float* tex, uint32_t material_count) {
    hipLaunchKernelGGL(k_guide_fold_bins, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, hits, fold, blob, tex, material_count);
}
void launch_bin_albedo_finish(uint32_t n_pixels, uint32_t bins, const float* sums, uint32_t samples, float* bin_albedo) {
    const size_t total = (size_t)bins * n_pixels;
    hipLaunchKernelGGL(k_bin_albedo_finish, dim3(line_grid(total)), dim3(kLine), 0, 0, total, sums, samples, bin_albedo);
}
void launch_dn_demodulate_bins(uint32_t n_pixels, uint32_t bins, const float* raw, const float* bin_albedo, const float* film, const uint32_t* counts, const double* stats,
                               float* out, float* color, uint8_t* flags) {
    if (bin_albedo)
        hipLaunchKernelGGL(k_dn_demodulate_bins<true>, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, bins, raw, bin_albedo, reinterpret_cast<const float4*>(film), counts,
                           reinterpret_cast<const double2*>(stats), out, reinterpret_cast<float4*>(color), flags);
    else
        hipLaunchKernelGGL(k_dn_demodulate_bins<false>, dim3(line_grid(n_pixels)), dim3(kLine), 0, 0, n_pixels, bins, raw, (const float*)nullptr,
                           reinterpret_cast<const float4*>(film), counts, reinterpret_cast<const double2*>(stats), out, reinterpret_cast<float4*>(color), flags);
}
void launch_dn_remodulate_bins(uint32_t n_pixels, uint32_t bins, const float* bin_albedo, const uint8_t* flags, float* spectral) {
    const size_t total = (size_t)bins * n_pixels;
    hipLaunchKernelGGL(k_dn_remodulate_bins, dim3(line_grid(total)), dim3(kLine), 0, 0, total, n_pixels, bin_albedo, flags, spectral);
}

}  // namespace ptk

extern "C" pt_status pt_denoise_spectral_albedo(const pt_denoise_desc* desc, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats,
                                                const float* guides, const float* albedo, const float* spectral, const float* bin_albedo, float* out_film,
                                                float* out_spectral, float* out_variance) {
    pt_denoise_desc d;
    std::string err;
    const pt_status st = pth::check_denoise_spectral_albedo_args(desc, bins, film, sample_counts, stats, guides, albedo, spectral, bin_albedo, out_film, out_spectral, &d, &err);
    if (st != PT_OK) return dfail(st, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return dfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
    if (d.device >= (uint32_t)ndev) return dfail(PT_ERR_INVALID_ARGUMENT, "device out of range");
#define DN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return dfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    DN_TRY(hipSetDevice((int)d.device));
    const size_t np = (size_t)d.width * d.height, bin_bytes = sizeof(float) * bins * np;
    Dev d_film, d_counts, d_stats, d_guides, d_color[2], d_geo, d_tent, d_flags, d_grad, d_var, d_bins[2], d_albedo, d_bin_albedo;
    DN_TRY(d_film.alloc(16 * np)); DN_TRY(d_counts.alloc(4 * np)); DN_TRY(d_stats.alloc(16 * np)); DN_TRY(d_guides.alloc(16 * np));
    DN_TRY(d_color[0].alloc(16 * np)); DN_TRY(d_color[1].alloc(16 * np)); DN_TRY(d_geo.alloc(16 * np)); DN_TRY(d_tent.alloc(4 * np));
    DN_TRY(d_flags.alloc(np)); DN_TRY(d_grad.alloc(8 * np)); DN_TRY(d_var.alloc(4 * np));
    DN_TRY(d_bins[0].alloc(bin_bytes)); DN_TRY(d_bins[1].alloc(bin_bytes));
    DN_TRY(hipMemcpy(d_film.p, film, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_counts.p, sample_counts, 4 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_stats.p, stats, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_guides.p, guides, 16 * np, hipMemcpyHostToDevice));
    DN_TRY(hipMemcpy(d_bins[1].p, spectral, bin_bytes, hipMemcpyHostToDevice));   // (the second ping-pong buffer is free until the first pass writes it)
    if (albedo) { DN_TRY(d_albedo.alloc(16 * np)); DN_TRY(hipMemcpy(d_albedo.p, albedo, 16 * np, hipMemcpyHostToDevice)); }
    if (bin_albedo) { DN_TRY(d_bin_albedo.alloc(bin_bytes)); DN_TRY(hipMemcpy(d_bin_albedo.p, bin_albedo, bin_bytes, hipMemcpyHostToDevice)); }
    DnParams P;
    P.width = d.width; P.height = d.height; P.sigma_l = d.sigma_luminance; P.sigma_z = d.sigma_depth; P.normal_squarings = d.normal_power_log2;
    if (albedo)
        ptk::launch_dn_prepare_albedo(P, d_film.as<float>(), d_counts.as<uint32_t>(), d_stats.as<double>(), d_guides.as<float>(), d_albedo.as<float>(), d_color[0].as<float>(),
                                      d_geo.as<float>(), d_flags.as<uint8_t>(), d_grad.as<float>());
    else
        ptk::launch_dn_prepare(P, d_film.as<float>(), d_counts.as<uint32_t>(), d_stats.as<double>(), d_guides.as<float>(), d_color[0].as<float>(), d_geo.as<float>(),
                               d_flags.as<uint8_t>(), d_grad.as<float>());
    ptk::launch_dn_demodulate_bins((uint32_t)np, bins, d_bins[1].as<float>(), d_bin_albedo.as<float>(), d_film.as<float>(), d_counts.as<uint32_t>(), d_stats.as<double>(),
                                   d_bins[0].as<float>(), d_color[0].as<float>(), d_flags.as<uint8_t>());
    int cur = 0;
    for (uint32_t i = 0; i < d.iterations; ++i) {
        ptk::launch_dn_tent(P, d_color[cur].as<float>(), d_geo.as<float>(), d_flags.as<uint8_t>(), d_tent.as<float>());
        ptk::launch_dn_gather_spectral(P, 1 << i, d_color[cur].as<float>(), d_geo.as<float>(), d_tent.as<float>(), d_flags.as<uint8_t>(), d_grad.as<float>(), bins,
                                       d_bins[cur].as<float>(), d_color[cur ^ 1].as<float>(), d_bins[cur ^ 1].as<float>());
        cur ^= 1;
    }
    if (albedo) ptk::launch_dn_finish_albedo((uint32_t)np, d_color[cur].as<float>(), d_albedo.as<float>(), d_flags.as<uint8_t>(), d_film.as<float>(), d_var.as<float>());
    else ptk::launch_dn_finish((uint32_t)np, d_color[cur].as<float>(), d_film.as<float>(), d_var.as<float>());
    if (bin_albedo) ptk::launch_dn_remodulate_bins((uint32_t)np, bins, d_bin_albedo.as<float>(), d_flags.as<uint8_t>(), d_bins[cur].as<float>());
    DN_TRY(hipGetLastError());
    DN_TRY(hipDeviceSynchronize());
    DN_TRY(hipMemcpy(out_film, d_film.p, 16 * np, hipMemcpyDeviceToHost));
    DN_TRY(hipMemcpy(out_spectral, d_bins[cur].p, bin_bytes, hipMemcpyDeviceToHost));
    if (out_variance) DN_TRY(hipMemcpy(out_variance, d_var.p, 4 * np, hipMemcpyDeviceToHost));
#undef DN_TRY
    return PT_OK;
}
