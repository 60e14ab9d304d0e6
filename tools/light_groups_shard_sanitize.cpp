// light_groups_shard_sanitize.cpp — a stand-alone host program for a sanitizer run of the packed group shard's rule (csrc/pt_light_groups_shard_rules.h, DESIGN.md
// section 15 "On every device of a node"): it packs, scatters and unpacks every shard of the films, shard counts and group counts that
// tests/test_light_groups_multi.py uses, in heap buffers of exactly the sizes the engine allocates, so that an index one past a group film or a packed film is a
// heap overflow the sanitizer sees.  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/light_groups_shard_sanitize tools/light_groups_shard_sanitize.cpp rust-pathtracer_amd/csrc/pt_plan.cpp && /tmp/light_groups_shard_sanitize
// It prints one line per film and "ok" at the end; a mismatch or an unwritten pixel ends it with status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../rust-pathtracer_amd/csrc/pt_light_groups_shard_rules.h"

using ptd::LgPixel;

int main() {
    const uint32_t films[4][2] = {{77, 45}, {40, 20}, {32, 32}, {1, 1}}, shards[5] = {1, 2, 3, 4, 8}, group_counts[3] = {1, 3, 8};
    uint32_t state = 12345u;
    for (const auto& f : films) {
        const uint32_t w = f[0], h = f[1], npx = w * h;
        size_t moved = 0;
        for (uint32_t n : shards)
            for (uint32_t G : group_counts) {
                std::vector<LgPixel> group_films((size_t)G * npx), scattered((size_t)G * npx), unpacked((size_t)G * npx);
                const auto put = [](float* dst, uint32_t word) { memcpy(dst, &word, sizeof word); };
                for (LgPixel& p : group_films) for (float& v : p.v) { state = state * 1664525u + 1013904223u; put(&v, state); }   // (any bit pattern: NaNs and infinities among them)
                for (std::vector<LgPixel>* back : {&scattered, &unpacked}) for (LgPixel& p : *back) for (float& v : p.v) put(&v, 0xDEADBEEFu);
                put(&group_films[0].v[0], 0x80000000u); put(&group_films.back().v[3], 0x7FC12345u);                                 // (-0.0, a NaN with a payload)
                std::vector<uint8_t> written(npx, 0);
                for (uint32_t v = 0; v < n; ++v) {
                    const std::vector<uint32_t> px = pth::shard_pixels(w, h, 32, 32, n > 1 ? v : 0u, n > 1 ? n : 0u);
                    if (px.empty()) continue;   // (a shard without a pixel launches nothing and copies nothing)
                    const uint32_t n_own = (uint32_t)px.size();
                    std::vector<LgPixel> packed((size_t)G * n_own);
                    for (uint32_t i = 0; i < n_own; ++i) ptd::lg_shard_pack_item(group_films.data(), npx, px.data(), n_own, G, i, packed.data());
                    ptd::lg_shard_scatter(packed.data(), px.data(), n_own, G, scattered.data(), npx);
                    for (uint32_t i = 0; i < n_own; ++i) ptd::lg_shard_unpack_item(packed.data(), px.data(), n_own, G, i, unpacked.data(), npx);
                    for (uint32_t p : px) ++written[p];
                    moved += packed.size();
                }
                for (uint32_t p = 0; p < npx; ++p) if (written[p] != 1) { printf("%ux%u n=%u: pixel %u is in %u shards\n", w, h, n, p, written[p]); return 1; }
                if (memcmp(group_films.data(), scattered.data(), sizeof(LgPixel) * group_films.size()) != 0) { printf("%ux%u n=%u G=%u: the scattered films came back changed\n", w, h, n, G); return 1; }
                if (memcmp(group_films.data(), unpacked.data(), sizeof(LgPixel) * group_films.size()) != 0) { printf("%ux%u n=%u G=%u: the unpacked films came back changed\n", w, h, n, G); return 1; }
            }
        printf("%ux%u: %zu pixels packed, scattered and unpacked, every pixel in one shard, every bit back\n", w, h, moved);
    }
    printf("ok\n");
    return 0;
}
