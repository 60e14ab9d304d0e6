// spectral_shard_sanitize.cpp — a stand-alone host program for a sanitizer run of the packed shard's rule (csrc/pt_spectral_shard_rules.h):
// it packs and scatters every shard of the films, shard counts and bin counts that tests/test_spectral_multi.py uses, in buffers of exactly the sizes the
// engine allocates, so that an index one past a plane or a packed plane is a heap overflow the sanitizer sees.  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/spectral_shard_sanitize tools/spectral_shard_sanitize.cpp rust-pathtracer_amd/csrc/pt_plan.cpp && /tmp/spectral_shard_sanitize
// It prints one line per film and "ok" at the end; a mismatch or an unwritten float ends it with status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../rust-pathtracer_amd/csrc/pt_spectral_shard_rules.h"

int main() {
    const uint32_t films[4][2] = {{77, 45}, {40, 20}, {32, 32}, {1, 1}}, shards[5] = {1, 2, 3, 4, 8}, bin_counts[3] = {1, 5, 64};
    uint32_t state = 12345u;
    for (const auto& f : films) {
        const uint32_t w = f[0], h = f[1], npx = w * h;
        size_t moved = 0;
        for (uint32_t n : shards)
            for (uint32_t bins : bin_counts) {
                std::vector<float> planes((size_t)bins * npx), back((size_t)bins * npx);
                const auto put = [](float* dst, uint32_t word) { memcpy(dst, &word, sizeof word); };
                for (float& v : planes) { state = state * 1664525u + 1013904223u; put(&v, state); }   // (any bit pattern: NaNs and infinities among them)
                for (float& v : back) put(&v, 0xDEADBEEFu);
                put(&planes[0], 0x80000000u); put(&planes.back(), 0x7FC12345u);                        // (-0.0, a NaN with a payload)
                std::vector<uint8_t> written(npx, 0);
                for (uint32_t v = 0; v < n; ++v) {
                    const std::vector<uint32_t> px = pth::shard_pixels(w, h, 32, 32, n > 1 ? v : 0u, n > 1 ? n : 0u);
                    if (px.empty()) continue;
                    std::vector<float> packed((size_t)bins * px.size());
                    for (uint32_t i = 0; i < px.size(); ++i) ptd::spectral_shard_pack_item(planes.data(), npx, px.data(), (uint32_t)px.size(), bins, i, packed.data());
                    ptd::spectral_shard_scatter(packed.data(), px.data(), (uint32_t)px.size(), bins, back.data(), npx);
                    for (uint32_t p : px) ++written[p];
                    moved += packed.size();
                }
                for (uint32_t p = 0; p < npx; ++p) if (written[p] != 1) { printf("%ux%u n=%u: pixel %u is in %u shards\n", w, h, n, p, written[p]); return 1; }
                if (memcmp(planes.data(), back.data(), sizeof(float) * planes.size()) != 0) { printf("%ux%u n=%u bins=%u: the planes came back changed\n", w, h, n, bins); return 1; }
            }
        printf("%ux%u: %zu floats packed and scattered, every pixel in one shard, every bit back\n", w, h, moved);
    }
    printf("ok\n");
    return 0;
}
