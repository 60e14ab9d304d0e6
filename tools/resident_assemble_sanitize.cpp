// resident_assemble_sanitize.cpp — the pack and unpack rules of a shard's spectral film (csrc/pt_spectral_shard_rules.h: what k_spectral_pack and
// k_spectral_unpack run lane after lane) over the shapes of tests/test_resident_assemble.py, in heap buffers of exactly the size the engine allocates, so that
// an index past a rule's range is an access past an allocation.  A host program of its own: build it with the sanitizers and run it,
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Irust-pathtracer_amd/csrc tools/resident_assemble_sanitize.cpp \
//       rust-pathtracer_amd/csrc/pt_plan.cpp -o /tmp/resident_assemble_sanitize && /tmp/resident_assemble_sanitize
//
// It packs every shard of random planes, unpacks the shards in reversed order into planes filled with a sentinel, and compares bit for bit; exit status 0 and
// the last line "ok" mean that nothing differed (the sanitizers end the program themselves on a bad access).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pt_plan.h"
#include "pt_spectral_shard_rules.h"

int main() {
    const uint32_t films[][2] = {{77, 45}, {40, 20}, {32, 32}, {1, 1}};
    const uint32_t shard_counts[] = {1, 2, 3, 4, 8}, bin_counts[] = {1, 5, 13, 64};
    uint64_t state = 0x9E3779B97F4A7C15ull, cases = 0;
    for (const auto& f : films)
        for (uint32_t n : shard_counts)
            for (uint32_t bins : bin_counts) {
                const uint32_t w = f[0], h = f[1];
                const size_t np = (size_t)w * h;
                std::unique_ptr<uint32_t[]> planes(new uint32_t[bins * np]), back(new uint32_t[bins * np]);
                for (size_t i = 0; i < bins * np; ++i) {   // (xorshift: every bit pattern, NaNs among them)
                    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
                    planes[i] = (uint32_t)(state >> 16);
                    back[i] = 0xDEADBEEFu;
                }
                planes[0] = 0x80000000u; planes[bins * np - 1] = 0x7FC12345u;
                std::vector<std::vector<uint32_t>> lists;
                std::vector<std::unique_ptr<uint32_t[]>> packed;
                for (uint32_t v = 0; v < n; ++v) {
                    lists.push_back(pth::shard_pixels(w, h, 32, 32, n > 1 ? v : 0u, n > 1 ? n : 0u));
                    const uint32_t n_own = (uint32_t)lists.back().size();
                    packed.emplace_back(new uint32_t[(size_t)bins * n_own]);   // (exactly the shard's size; an empty shard has none)
                    for (uint32_t i = 0; i < n_own; ++i)
                        ptd::spectral_shard_pack_item(reinterpret_cast<const float*>(planes.get()), np, lists.back().data(), n_own, bins, i, reinterpret_cast<float*>(packed.back().get()));
                }
                for (uint32_t v = n; v-- > 0;) {
                    const uint32_t n_own = (uint32_t)lists[v].size();
                    for (uint32_t i = 0; i < n_own; ++i)
                        ptd::spectral_shard_unpack_item(reinterpret_cast<const float*>(packed[v].get()), lists[v].data(), n_own, bins, i, reinterpret_cast<float*>(back.get()), np);
                }
                if (std::memcmp(planes.get(), back.get(), sizeof(uint32_t) * bins * np) != 0) {
                    fprintf(stderr, "%ux%u, %u shards, %u bins: the unpacked planes differ\n", w, h, n, bins);
                    return 1;
                }
                ++cases;
            }
    printf("%llu cases\nok\n", (unsigned long long)cases);
    return 0;
}
