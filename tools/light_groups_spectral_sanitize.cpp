// light_groups_spectral_sanitize.cpp — a stand-alone host program for a sanitizer run of the rules of spectral light groups
// (csrc/pt_light_groups_spectral_rules.h): it runs the fold of k_accumulate_group_bins, the re-lamp matrix and the re-lamp rule over the
// sizes tests/test_light_groups_spectral.py uses, in heap buffers of exactly the sizes the engine allocates — 2 + G energy planes of `capacity` floats, G * bins
// planes of width x height floats, K x G x bins weights, K planes of output — so that an index one past a plane is a heap overflow the sanitizer sees.  The
// fold's accumulators sit in a column of a block-sized array indexed as the kernel indexes its LDS (b * block + lane).  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/lgs_sanitize tools/light_groups_spectral_sanitize.cpp rust-pathtracer_amd/csrc/pt_scene_host.cpp rust-pathtracer_amd/csrc/pt_plan.cpp && /tmp/lgs_sanitize
// It prints one line per case and "ok" at the end; a fold that differs from the sum made sample by sample, a kept group's rows that are not
// pt_spectral_response_matrix's or a re-lamp that differs from the plain fold ends it with status 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_light_groups_spectral_rules.h"
#include "../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../rust-pathtracer_amd/csrc/pt_scene_host.h"

using namespace ptd;

namespace {
uint32_t state = 2463534242u;
float rnd() { state ^= state << 13; state ^= state >> 17; state ^= state << 5; return (float)(state >> 8) * (1.0f / 16777216.0f); }
bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0; }

template <int KC>
void relamp_rows(uint32_t n_pixels, uint32_t planes, const float* matrix, const float* gs, float* out) {
    for (uint32_t p = 0; p < n_pixels; ++p)
        spectral_project_pixel<KC>(
            planes, [&](uint32_t i) { return gs[(size_t)i * n_pixels + p]; }, [&](int k, uint32_t i) { return matrix[(uint32_t)k * planes + i]; },
            [&](int k, float v) { out[(size_t)k * n_pixels + p] = v; });
}
}  // namespace

int main() {
    const uint32_t films[3][2] = {{17, 13}, {24, 24}, {64, 4}}, groups[3] = {1, 3, 8}, bin_counts[3] = {1, 5, 64}, ks[4] = {1, 3, 9, 16};
    constexpr uint32_t kBlock = 256;
    // ---- the fold: passes of `chunk` pixels x up to 10 samples over a film, as the pass loop makes them
    for (const auto& f : films)
        for (uint32_t G : groups)
            for (uint32_t bins : bin_counts) {
                const uint32_t np = f[0] * f[1], spp = 23, chunk = 97, capacity = chunk * 10;
                std::vector<float> energy((size_t)lg_planes(G) * capacity), gs((size_t)G * bins * np, 0.0f), want((size_t)G * bins * np, 0.0f), lds((size_t)bins * kBlock);
                RenderParams rp;
                memset(&rp, 0, sizeof(rp));
                rp.wavelength_lo = 380.0f; rp.wavelength_span = 400.0f; rp.spp = spp; rp.range_end = spp; rp.normalize = 1u; rp.energy_stride = capacity;
                for (uint32_t begin = 0; begin < np; begin += chunk)
                    for (uint32_t first = 0; first < spp; first += 10) {
                        rp.chunk_pixels = np - begin < chunk ? np - begin : chunk; rp.first_sample = first; rp.pass_samples = spp - first < 10 ? spp - first : 10;
                        const uint32_t n = rp.chunk_pixels * rp.pass_samples;
                        for (uint32_t i = 0; i < n; ++i) {
                            energy[i] = 0.0f; energy[(size_t)capacity + i] = rnd();
                            for (uint32_t g = 0; g < G; ++g) energy[(size_t)lg_plane(g) * capacity + i] = rnd() < 0.3f ? 0.0f : rnd();
                        }
                        for (uint32_t g = 0; g < G; ++g)
                            for (uint32_t p = 0; p < rp.chunk_pixels; ++p) {
                                const uint32_t pixel = begin + p, lane = p % kBlock;
                                float* px = gs.data() + (size_t)g * bins * np + pixel;
                                for (uint32_t b = 0; b < bins; ++b) lds[(size_t)b * kBlock + lane] = px[(size_t)b * np];
                                lg_spectral_fold_pixel(rp, bins, energy.data(), g, p, [&](uint32_t b) -> float& { return lds[(size_t)b * kBlock + lane]; });
                                for (uint32_t b = 0; b < bins; ++b) px[(size_t)b * np] = lds[(size_t)b * kBlock + lane];
                                // the same sum, sample by sample, straight into the planes
                                float* wx = want.data() + (size_t)g * bins * np + pixel;
                                for (uint32_t s = 0; s < rp.pass_samples; ++s) {
                                    const size_t slot = (size_t)s * rp.chunk_pixels + p;
                                    const float lambda = rp.wavelength_lo + energy[(size_t)capacity + slot] * rp.wavelength_span;
                                    wx[(size_t)spectral_bin(rp.wavelength_lo, rp.wavelength_span, bins, lambda) * np] += energy[(size_t)lg_plane(g) * capacity + slot];
                                }
                                if (first + rp.pass_samples == spp) for (uint32_t b = 0; b < bins; ++b) wx[(size_t)b * np] /= (float)spp;
                            }
                    }
                if (!same(gs, want)) { printf("%ux%u G=%u bins=%u: the fold differs from the sum made sample by sample\n", f[0], f[1], G, bins); return 1; }
                printf("%ux%u G=%u bins=%u: the fold over %u passes is the sample-by-sample sum\n", f[0], f[1], G, bins, ((np + chunk - 1) / chunk) * 3);
            }
    // ---- the matrix: curves of four kinds, a kept group, a flat pair, an old curve with zeros
    {
        const float data[] = {5.0f, 10.0f, 380.0f, 0.0f, 450.0f, 0.0f, 500.0f, 2.0f, 600.0f, 0.0f, 780.0f, 1.0f};
        pt_curve curves[4];
        memset(curves, 0, sizeof(curves));
        curves[0].kind = PT_CURVE_LINEAR; curves[0].p0 = 370.0f; curves[0].p1 = 790.0f; curves[0].data_offset = 0; curves[0].data_count = 1;   // flat 5
        curves[1] = curves[0]; curves[1].data_offset = 1;                                                                                     // flat 10
        curves[2].kind = PT_CURVE_TABULATED; curves[2].data_offset = 2; curves[2].data_count = 5;                                             // with zeros
        curves[3].kind = PT_CURVE_BLACKBODY; curves[3].p0 = 3000.0f; curves[3].p1 = 5.0f;
        pt_render_desc rd;
        memset(&rd, 0, sizeof(rd));
        rd.wavelength_lo = 380.0f; rd.wavelength_hi = 780.0f;
        for (uint32_t bins : bin_counts)
            for (uint32_t n : {1u, 16u}) {
                const pt_spectral_desc sd = {bins, {0u, 0u, 0u}};
                const int32_t responses[4] = {PT_RESPONSE_CIE_X, PT_RESPONSE_CIE_Y, PT_RESPONSE_CIE_Z, 3}, old_curve[3] = {PT_RELAMP_KEEP, 0, 2}, new_curve[3] = {PT_RELAMP_KEEP, 1, 3};
                const float gain[3] = {1.0f, 1.0f, -0.5f};
                std::vector<float> W((size_t)4 * 3 * bins), R((size_t)4 * bins);
                std::string err;
                if (pth::light_groups_relamp_matrix(&rd, &sd, curves, 4, data, 12, 4, responses, 2, n, 3, old_curve, new_curve, gain, W.data(), &err) != PT_OK ||
                    !pth::spectral_response_matrix(380.0f, 780.0f, bins, curves, 4, data, 12, 4, responses, 2, n, R.data(), &err)) { printf("matrix: %s\n", err.c_str()); return 1; }
                for (uint32_t k = 0; k < 4; ++k)
                    for (uint32_t b = 0; b < bins; ++b) {
                        const float kept = W[((size_t)k * 3 + 0) * bins + b], twice = W[((size_t)k * 3 + 1) * bins + b], r = R[(size_t)k * bins + b], r2 = 2.0f * r;
                        if (memcmp(&kept, &r, 4) != 0 || memcmp(&twice, &r2, 4) != 0) { printf("bins=%u n=%u: a kept or doubled row differs at %u, %u\n", bins, n, k, b); return 1; }
                    }
                printf("matrix bins=%u subsamples=%u: kept rows are the response matrix's, E5 -> E10 doubles them\n", bins, n);
            }
    }
    // ---- the re-lamp: the launcher's grouping against the plain fold
    for (const auto& f : films)
        for (uint32_t G : groups)
            for (uint32_t bins : bin_counts)
                for (uint32_t K : ks) {
                    const uint32_t np = f[0] * f[1], planes = G * bins;
                    std::vector<float> gs((size_t)planes * np), W((size_t)K * planes), out((size_t)K * np), want((size_t)K * np);
                    for (float& v : gs) v = rnd() * 4.0f - 1.0f;
                    for (float& v : W) v = rnd() < 0.2f ? 0.0f : rnd() * 4.0f - 2.0f;
                    std::string err;
                    if (pth::check_relamp_args(f[0], f[1], G, bins, K, W.data(), gs.data(), out.data(), &err) != PT_OK) { printf("check: %s\n", err.c_str()); return 1; }
                    for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)SP_CHUNK) {
                        const float* m = W.data() + (size_t)k0 * planes;
                        float* o = out.data() + (size_t)k0 * np;
                        switch (K - k0 < (uint32_t)SP_CHUNK ? K - k0 : (uint32_t)SP_CHUNK) {
                            case 1: relamp_rows<1>(np, planes, m, gs.data(), o); break;
                            case 3: relamp_rows<3>(np, planes, m, gs.data(), o); break;
                            default: relamp_rows<8>(np, planes, m, gs.data(), o); break;
                        }
                    }
                    for (uint32_t k = 0; k < K; ++k)
                        for (uint32_t p = 0; p < np; ++p) {
                            float acc = 0.0f;
                            for (uint32_t i = 0; i < planes; ++i) acc = acc + W[(size_t)k * planes + i] * gs[(size_t)i * np + p];
                            want[(size_t)k * np + p] = acc;
                        }
                    if (!same(out, want)) { printf("%ux%u G=%u bins=%u K=%u: the re-lamp differs from the plain fold\n", f[0], f[1], G, bins, K); return 1; }
                }
    printf("re-lamp: every size, G, bin count and K equals the plain fold\n");
    printf("ok\n");
    return 0;
}
