// matte_sanitize.cpp — a stand-alone host program for a sanitizer run of the rules of ID mattes (csrc/pt_matte_rules.h): it runs the fold,
// the finish, the extract and the hash over the sizes tests/test_matte.py uses, in heap buffers of exactly the sizes the engine allocates — the plane-major slot
// table of n x (8 R + 4) bytes with the overflow plane behind the slots, R planes of keys and of coverage, 17 offsets and the selected keys, M planes of output —
// indexed as the kernels index them (slot r of pixel p at r * n + p), so that an index one past a plane is a heap overflow the sanitizer sees.  From the
// repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/matte_sanitize tools/matte_sanitize.cpp rust-pathtracer_amd/csrc/pt_scene_host.cpp rust-pathtracer_amd/csrc/pt_plan.cpp && /tmp/matte_sanitize
// It prints one line per case and "ok" at the end; a fold that breaks sum of counts + overflow = S, ranks out of order, an extract that differs from a linear
// search, a network that fails one of the 256 zero-one inputs or a hash that misses its vector ends it with status 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_matte_rules.h"
#include "../rust-pathtracer_amd/csrc/pt_plan.h"

using namespace ptd;

namespace {
uint32_t state = 2463534242u;
uint32_t rnd(uint32_t n) { state ^= state << 13; state ^= state >> 17; state ^= state << 5; return (state >> 8) % n; }
int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

// one film through the three kernels' loops for a constant R: 0 = fine
template <int R>
int run(uint32_t w, uint32_t h, uint32_t S, uint32_t distinct) {
    const uint32_t n = w * h;
    std::vector<char> table((size_t)n * (8u * R + 4u));
    MatteSlot* slots = reinterpret_cast<MatteSlot*>(table.data());
    uint32_t* overflow = reinterpret_cast<uint32_t*>(table.data() + 8u * (size_t)R * n);
    std::vector<uint32_t> sample_keys((size_t)S * n);
    for (uint32_t k = 0; k < S; ++k) {
        for (uint32_t p = 0; p < n; ++p) {   // the fold kernel's lane p of launch k
            const uint32_t pick = rnd(distinct + 1u);
            const uint32_t key = matte_sample_key(pick != distinct, 7u + pick, (1u << 16) | pick, p & 1u);
            sample_keys[(size_t)k * n + p] = key;
            if (k == 0) {
                slots[p] = MatteSlot{key, 1u};
                for (int r = 1; r < R; ++r) slots[(size_t)r * n + p] = MatteSlot{0u, 0u};
                overflow[p] = 0u;
                continue;
            }
            MatteSlot s[R];
            for (int r = 0; r < R; ++r) s[r] = slots[(size_t)r * n + p];
            const int slot = matte_fold_slot<R>(s, key);
            if (slot == R) overflow[p] += 1u; else slots[(size_t)slot * n + p] = matte_fold_value<R>(s, slot, key);
        }
    }
    std::vector<uint32_t> keys((size_t)R * n), over(n);
    std::vector<float> coverage((size_t)R * n);
    for (uint32_t p = 0; p < n; ++p) {   // the finish kernel's lane p
        MatteSlot s[R];
        for (int r = 0; r < R; ++r) s[r] = slots[(size_t)r * n + p];
        uint32_t k[R];
        float c[R];
        matte_finish_pixel<R>(s, S, k, c);
        uint32_t total = overflow[p];
        for (int r = 0; r < R; ++r) {
            keys[(size_t)r * n + p] = k[r]; coverage[(size_t)r * n + p] = c[r];
            uint32_t seen = 0;
            for (uint32_t q = 0; q < S; ++q) seen += sample_keys[(size_t)q * n + p] == k[r] ? 1u : 0u;
            if (k[r] == MATTE_NONE ? c[r] != 0.0f : !(c[r] > 0.0f && c[r] <= (float)seen / (float)S)) return fail("a rank's coverage is not its key's share");
            if (r > 0 && (c[r] > c[r - 1] || (c[r] == c[r - 1] && k[r] != MATTE_NONE && k[r] <= k[r - 1]))) return fail("ranks out of order");
            total += (uint32_t)(c[r] * (float)S + 0.5f);
        }
        over[p] = overflow[p];
        if (total != S) return fail("sum of counts + overflow != S");
    }
    // the extract: every set of a 16-set selection against a linear search of the raw selection
    std::vector<uint32_t> offsets(1, 0u), selected;
    for (uint32_t m = 0; m < MATTE_SETS_MAX; ++m) {
        const uint32_t count = m == 0 ? 0u : rnd(64u);
        for (uint32_t i = 0; i < count; ++i) selected.push_back(rnd(4u) == 0 ? MATTE_SKY : (rnd(2u) ? 7u + rnd(distinct + 2u) : (1u << 16) | rnd(distinct + 2u)));
        offsets.push_back((uint32_t)selected.size());
    }
    std::string err;
    if (pth::check_matte_extract_args(w, h, R, keys.data(), coverage.data(), MATTE_SETS_MAX, offsets.data(), selected.data(), keys.data(), &err) != PT_OK) return fail(err.c_str());
    std::vector<uint32_t> words;
    pth::matte_selection_words(MATTE_SETS_MAX, offsets.data(), selected.data(), &words);
    std::vector<uint32_t> staged_offsets(words.begin(), words.begin() + MATTE_SETS_MAX + 1u), staged(words.begin() + MATTE_SETS_MAX + 1u, words.end());   // (the kernel's two LDS arrays, of their exact sizes)
    std::vector<float> out((size_t)MATTE_SETS_MAX * n);
    for (uint32_t p = 0; p < n; ++p) {   // the extract kernel's lane p
        uint32_t k[R];
        float c[R];
        for (int r = 0; r < R; ++r) { k[r] = keys[(size_t)r * n + p]; c[r] = coverage[(size_t)r * n + p]; }
        for (uint32_t m = 0; m < MATTE_SETS_MAX; ++m) {
            out[(size_t)m * n + p] = matte_extract_pixel<R>(k, c, staged.data(), staged_offsets[m], staged_offsets[m + 1]);
            float want = 0.0f;
            for (int r = 0; r < R; ++r) {
                bool in = false;
                for (uint32_t i = offsets[m]; i < offsets[m + 1]; ++i) in = in || (selected[i] == k[r] && k[r] != MATTE_NONE);
                if (in) want = want + c[r];
            }
            if (memcmp(&want, &out[(size_t)m * n + p], 4) != 0) return fail("the extract differs from a linear search");
        }
    }
    printf("%ux%u S=%u R=%d, %u keys: fold, finish, extract of 16 sets (%zu keys staged)\n", w, h, S, R, distinct, staged.size());
    return 0;
}
}  // namespace

int main() {
    int bad = 0;
    bad |= run<1>(40, 27, 5, 3); bad |= run<2>(40, 27, 5, 3); bad |= run<3>(24, 16, 4, 2); bad |= run<4>(17, 13, 9, 6); bad |= run<5>(5, 3, 65, 9);
    bad |= run<6>(40, 27, 5, 4); bad |= run<7>(1, 1, 300, 12); bad |= run<8>(32, 24, 6, 11);
    if (bad) return 1;
    // the sorting network on every zero-one input
    for (uint32_t pattern = 0; pattern < 256u; ++pattern) {
        uint64_t v[8];
        for (int i = 0; i < 8; ++i) v[i] = (pattern >> i) & 1u;
        matte_sort8(v);
        for (int i = 1; i < 8; ++i) if (v[i - 1] > v[i]) return fail("the network leaves a zero-one input unsorted");
    }
    printf("sorting network: 256 zero-one inputs\n");
    // the hash: the vectors of DESIGN.md section 16, every tail length, the exponent fix
    const struct { const char* name; uint32_t hash; } vectors[] = {{"", 0u}, {"hello", 0x248bfa47u}, {"Hello, world!", 0xc0363e43u}, {"instance0", 0x1aff6f28u},
                                                                   {"lambertian_white", 0x0dd41c3cu}, {"CryptoObject", 0x3ae39a58u}};
    for (const auto& v : vectors) {
        const std::vector<uint8_t> bytes(v.name, v.name + strlen(v.name));   // (a heap copy of exactly the name's length: a read past the tail is seen)
        if (matte_murmur3_32(bytes.data(), bytes.size(), 0u) != v.hash) return fail(v.name);
    }
    const std::vector<uint8_t> ff(4, 0xffu), hw{'H', 'e', 'l', 'l', 'o', ',', ' ', 'w', 'o', 'r', 'l', 'd', '!'};
    if (matte_murmur3_32(hw.data(), hw.size(), 1234u) != 0xfaf6cdb3u || matte_murmur3_32(ff.data(), 0, 1u) != 0x514e28b7u || matte_murmur3_32(ff.data(), 4, 0u) != 0x76293b50u)
        return fail("a seeded hash vector");
    if (matte_id_bits(0u) != 0x00800000u || matte_id_bits(0x7f800001u) != 0x7f000001u || matte_id_bits(0xff812345u) != 0xff012345u || matte_id_bits(0x3ae39a58u) != 0x3ae39a58u)
        return fail("the exponent fix");
    printf("hash: 9 vectors, the exponent fix\n");
    // the argument checks the engine and the emulation share
    std::string err;
    const uint32_t off_bad[4] = {0, 5, 4, 6}, off_big[3] = {0, 600, 1025}, sel[8] = {0};
    if (pth::check_matte_selections(17, off_bad, sel, sel, &err) == PT_OK || pth::check_matte_selections(3, off_bad, sel, sel, &err) == PT_OK ||
        pth::check_matte_selections(2, off_big, sel, sel, &err) == PT_OK)
        return fail("a bad selection passed");
    printf("ok\n");
    return 0;
}
