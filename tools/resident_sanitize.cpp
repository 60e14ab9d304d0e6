// resident_sanitize.cpp — a stand-alone host program for a sanitizer run of the resident filter's rules (csrc/pt_denoise_resident_rules.h):
// it runs the interleave and de-interleave index rule and the quad gather rule over the film sizes and bin counts that tests/test_denoise_resident.py uses,
// in heap buffers of exactly the sizes the engine allocates — Q planes of width x height quads, B planes of width x height floats — so that an index one past
// a plane is a heap overflow the sanitizer sees.  Every tap of every pass is taken where it lies inside the film (the weights do not matter to an index), at
// the steps 1 .. 16 of five passes.  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/resident_sanitize tools/resident_sanitize.cpp && /tmp/resident_sanitize
// It prints one line per film and "ok" at the end; a round trip that changes a bit, a pad that is not +0.0f or a quad gather that differs from the plane-major
// one ends it with status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_denoise_resident_rules.h"

using namespace ptd;

namespace {
// a pass's source over exactly-sized buffers: the bins as planes and as quads (the film filter's members are not read by the bin rules)
struct Source {
    const float* planes; const DnQuad* quads; uint32_t width; size_t plane;
    float bin(uint32_t b, int x, int y) const { return planes[(size_t)b * plane + (size_t)y * width + (size_t)x]; }
    DnQuad bin4(uint32_t q, int x, int y) const { return quads[dn_quad_index(q, plane, (size_t)y * width + (size_t)x)]; }
};
}  // namespace

int main() {
    const uint32_t films[6][2] = {{64, 40}, {37, 53}, {5, 3}, {1, 9}, {9, 1}, {257, 3}}, bin_counts[11] = {1, 3, 4, 5, 7, 8, 9, 12, 13, 32, 64};
    uint32_t state = 2463534242u;
    for (const auto& f : films) {
        const uint32_t w = f[0], h = f[1];
        const size_t np = (size_t)w * h;
        size_t gathered = 0;
        for (uint32_t bins : bin_counts) {
            const uint32_t Q = dn_quad_count(bins);
            std::vector<float> planes((size_t)bins * np), back((size_t)bins * np), out_planes((size_t)bins * np);
            std::vector<DnQuad> quads((size_t)Q * np), out_quads((size_t)Q * np);
            for (float& v : planes) { state ^= state << 13; state ^= state >> 17; state ^= state << 5; v = (float)(state >> 8) * (1.0f / 16777216.0f); }
            for (size_t p = 0; p < np; ++p) {
                const uint32_t dead = dn_bins_to_quads_pixel(bins, 0u, [&](uint32_t b) { return planes[(size_t)b * np + p]; }, [](uint32_t) { return 1.0f; },
                                                             [&](uint32_t q, DnQuad v) { quads[dn_quad_index(q, np, p)] = v; });
                if (dead) { printf("%ux%u bins=%u: a finite pixel came out dead\n", w, h, bins); return 1; }
                dn_quads_to_bins_pixel<true>(bins, 0u, [&](uint32_t q) { return quads[dn_quad_index(q, np, p)]; }, [](uint32_t) { return 1.0f; },
                                             [&](uint32_t b, float v) { back[(size_t)b * np + p] = v; });
                for (uint32_t b = bins; b < 4u * Q; ++b) {
                    const float pad = quads[dn_quad_index(dn_quad_of_bin(b), np, p)][dn_quad_lane_of_bin(b)];
                    uint32_t word;
                    memcpy(&word, &pad, sizeof word);
                    if (word != 0u) { printf("%ux%u bins=%u: a pad bin is not +0.0f\n", w, h, bins); return 1; }
                }
            }
            if (memcmp(planes.data(), back.data(), sizeof(float) * planes.size()) != 0) { printf("%ux%u bins=%u: the round trip changed a bit\n", w, h, bins); return 1; }
            const Source src{planes.data(), quads.data(), w, np};
            for (int step = 1; step <= 16; step *= 2) {
                for (uint32_t y = 0; y < h; ++y)
                    for (uint32_t x = 0; x < w; ++x) {
                        DnTaps T;
                        T.mask = 0u; T.sw = 0.0f;
                        for (int dy = -2; dy <= 2; ++dy)
                            for (int dx = -2; dx <= 2; ++dx) {
                                const int t = (dy + 2) * 5 + (dx + 2), qx = (int)x + dx * step, qy = (int)y + dy * step;
                                T.w[t] = 0.0f;
                                if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) continue;
                                T.w[t] = 1.0f / (float)(1 + (t % 7));
                                T.mask |= 1u << t; T.sw = T.sw + T.w[t];
                            }
                        if ((x + y) % 11u == 10u) T.mask = 0u;   // (a dead pixel's path: its own quads copied through)
                        const size_t p = (size_t)y * w + x;
                        dn_gather_pixel_bins(src, step, (int)x, (int)y, T, bins, [&](uint32_t b, float v) { out_planes[(size_t)b * np + p] = v; });
                        dn_gather_pixel_bins4(src, step, (int)x, (int)y, T, Q, [&](uint32_t q, DnQuad v) { out_quads[dn_quad_index(q, np, p)] = v; });
                        for (uint32_t b = 0; b < bins; ++b) {
                            const float a = out_planes[(size_t)b * np + p], c = out_quads[dn_quad_index(dn_quad_of_bin(b), np, p)][dn_quad_lane_of_bin(b)];
                            if (memcmp(&a, &c, sizeof a) != 0) { printf("%ux%u bins=%u step=%d: bin %u of pixel %zu differs\n", w, h, bins, step, b, p); return 1; }
                        }
                        gathered += bins;
                    }
            }
        }
        printf("%ux%u: every bin count round-tripped, pads +0.0f, %zu gathered bins equal to the plane-major rule's\n", w, h, gathered);
    }
    printf("ok\n");
    return 0;
}
