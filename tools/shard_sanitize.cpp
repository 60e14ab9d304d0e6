// shard_sanitize.cpp — a stand-alone host program for a sanitizer run of the packed shard's rule (csrc/pt_shard_rules.h; DESIGN.md section 14, "Assembling a node
// render" and section 15 "On every device of a node"), in both of its elements: floats (the spectral film: what k_spectral_pack and k_spectral_unpack run lane
// after lane) and pixels of four floats (the group films: k_light_groups_pack, k_light_groups_unpack).  It packs every shard of the films, shard counts and plane
// counts that tests/test_spectral_multi.py, tests/test_resident_assemble.py and tests/test_light_groups_multi.py use, scatters the shards as the node entries' host
// threads do, and unpacks them item by item in reversed shard order as pt_resident_assemble may, in heap buffers of exactly the sizes the engine allocates, so
// that an index one past a plane or a packed plane is a heap overflow the sanitizer sees.  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/shard_sanitize tools/shard_sanitize.cpp rust-pathtracer_amd/csrc/pt_plan.cpp && /tmp/shard_sanitize
// It prints one line per film and "ok" at the end; a mismatch or a pixel that is not in exactly one shard ends it with status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../rust-pathtracer_amd/csrc/pt_shard_rules.h"

static uint32_t g_state = 12345u;

static void put(void* dst, size_t word, uint32_t value) { memcpy(static_cast<unsigned char*>(dst) + 4 * word, &value, sizeof value); }

// One film, shard count and plane count in elements Q: false (and a line that says why) when a pixel is not in exactly one shard or a bit came back changed
template <typename Q>
static bool round_trip(uint32_t w, uint32_t h, uint32_t n, uint32_t planes, size_t* moved) {
    const uint32_t npx = w * h;
    const size_t words = sizeof(Q) / 4 * planes * npx;
    std::vector<Q> full((size_t)planes * npx), scattered(full.size()), unpacked(full.size());
    for (size_t i = 0; i < words; ++i) {   // (any bit pattern: NaNs and infinities among them)
        g_state = g_state * 1664525u + 1013904223u;
        put(full.data(), i, g_state); put(scattered.data(), i, 0xDEADBEEFu); put(unpacked.data(), i, 0xDEADBEEFu);
    }
    put(full.data(), 0, 0x80000000u); put(full.data(), words - 1, 0x7FC12345u);   // (-0.0, a NaN with a payload)
    std::vector<uint8_t> written(npx, 0);
    std::vector<std::vector<uint32_t>> lists;
    std::vector<std::vector<Q>> packed;
    for (uint32_t v = 0; v < n; ++v) {
        lists.push_back(pth::shard_pixels(w, h, 32, 32, n > 1 ? v : 0u, n > 1 ? n : 0u));
        const std::vector<uint32_t>& px = lists.back();
        const uint32_t n_own = (uint32_t)px.size();
        packed.emplace_back((size_t)planes * n_own);   // (exactly the shard's size; a shard without a pixel has none, launches nothing and copies nothing)
        for (uint32_t i = 0; i < n_own; ++i) ptd::shard_pack_item(full.data(), npx, px.data(), n_own, planes, i, packed.back().data());
        if (n_own) ptd::shard_scatter(packed.back().data(), px.data(), n_own, planes, scattered.data(), npx);
        for (uint32_t p : px) ++written[p];
        *moved += packed.back().size();
    }
    for (uint32_t v = n; v-- > 0;)
        for (uint32_t i = 0; i < lists[v].size(); ++i) ptd::shard_unpack_item(packed[v].data(), lists[v].data(), (uint32_t)lists[v].size(), planes, i, unpacked.data(), npx);
    for (uint32_t p = 0; p < npx; ++p)
        if (written[p] != 1) { printf("%ux%u n=%u: pixel %u is in %u shards\n", w, h, n, p, written[p]); return false; }
    for (const std::vector<Q>* back : {&scattered, &unpacked})
        if (memcmp(full.data(), back->data(), sizeof(Q) * full.size()) != 0) {
            printf("%ux%u n=%u planes=%u of %zu floats: the %s planes came back changed\n", w, h, n, planes, sizeof(Q) / 4, back == &scattered ? "scattered" : "unpacked");
            return false;
        }
    return true;
}

int main() {
    const uint32_t films[4][2] = {{77, 45}, {40, 20}, {32, 32}, {1, 1}}, shards[5] = {1, 2, 3, 4, 8}, bin_counts[4] = {1, 5, 13, 64}, group_counts[3] = {1, 3, 8};
    for (const auto& f : films) {
        size_t floats = 0, pixels = 0;
        for (uint32_t n : shards) {
            for (uint32_t bins : bin_counts) if (!round_trip<float>(f[0], f[1], n, bins, &floats)) return 1;
            for (uint32_t G : group_counts) if (!round_trip<ptd::ShardPixel>(f[0], f[1], n, G, &pixels)) return 1;
        }
        printf("%ux%u: %zu floats and %zu pixels packed, scattered and unpacked, every pixel in one shard, every bit back\n", f[0], f[1], floats, pixels);
    }
    printf("ok\n");
    return 0;
}
