// pt_matte_rules.h — the rules of ID mattes (pt_render_mattes / pt_matte_extract / pt_cryptomatte_hash of include/pt_denoise.h) as
// PT_HD functions that the kernels (pt_matte.hip) and the host emulation of the tests (tests/host_emulation/ptemu_matte.cpp) both compile: one text, so they
// agree bit for bit.
//
// Key of a sample: camera sample k of pixel p (pt_camera_samples), traced as pt_intersect traces it; hit.instance or hit.material (the packed MaterialId),
// MATTE_SKY on a miss.
// Fold: a pixel owns R slots (key, count), all empty (count 0) at the start.  Samples are folded in k order, scanning the slots r = 0 .. R-1: the first slot
// that is empty takes (key, 1), a slot with the same key takes count + 1; with neither, the pixel's overflow count takes + 1 and the sample is dropped.  The
// slots fill from r = 0 and hold a key once, so "the first slot that is empty or holds the key" is the slot to change.
// Finish: the slots sorted by count descending, ties by key ascending; an empty slot becomes (MATTE_NONE, 0.0f), any other (key, (float)count / (float)S) —
// one IEEE f32 division.  sum of the counts + overflow = S.
// Extract: out = 0.0f; for r = 0 .. R-1 in rank order, out = out + coverage[r] where keys[r] is in the set.  MATTE_NONE is in no set.  Only membership and
// the order of the additions are fixed: any search is bit-exact.
// Cryptomatte id of a name: MurmurHash3_x86_32 of its bytes, seed 0; if the exponent field (h >> 23) & 255 is 0 or 255, bit 23 is flipped, so that the float
// with these bits is neither a denormal nor an infinity nor a NaN.
#ifndef PT_MATTE_RULES_H
#define PT_MATTE_RULES_H
#include <stddef.h>
#include <stdint.h>

#include "pt_device.h"

namespace ptd {

constexpr uint32_t MATTE_SKY = 0xFFFFFFFEu, MATTE_NONE = 0xFFFFFFFFu;   // PT_MATTE_SKY, PT_MATTE_NONE of the header
constexpr int MATTE_RANKS_MAX = 8;                                     // PT_MATTE_RANKS_MAX
constexpr uint32_t MATTE_SAMPLES_MAX = 65535u;
constexpr uint32_t MATTE_KEY_INSTANCE = 0u, MATTE_KEY_MATERIAL = 1u;   // PT_MATTE_KEY_*
constexpr uint32_t MATTE_SETS_MAX = 16u, MATTE_SELECTED_MAX = 1024u;   // the caps of an extract

struct alignas(8) MatteSlot { uint32_t key, count; };   // one 8-byte word of the slot table

PT_HD uint32_t matte_sample_key(int32_t valid, uint32_t instance, uint32_t material, uint32_t key_kind) {
    if (!valid) return MATTE_SKY;
    return key_kind == MATTE_KEY_MATERIAL ? material : instance;
}

// The slot of s[0 .. R-1] that sample `key` changes, R when it overflows.  Every index into s is a constant after unrolling.
template <int R>
PT_HD int matte_fold_slot(const MatteSlot (&s)[R], uint32_t key) {
    int slot = R;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) if (s[r].count == 0u || s[r].key == key) slot = r;
    return slot;
}
// ... and what that slot holds afterwards
template <int R>
PT_HD MatteSlot matte_fold_value(const MatteSlot (&s)[R], int slot, uint32_t key) {
    uint32_t count = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) if (r == slot) count = s[r].count;
    return MatteSlot{key, count + 1u};
}

// The order of the finish as one ascending 64-bit word: the count's complement above the key (count descending, then key ascending; MATTE_SKY sorts as its
// value).  An empty slot is (MATTE_NONE, 0): behind every other.
PT_HD uint64_t matte_order_word(MatteSlot s) {
    const uint32_t key = s.count == 0u ? MATTE_NONE : s.key;
    return ((uint64_t)(~s.count) << 32) | (uint64_t)key;
}
PT_HD void matte_compare_exchange(uint64_t* a, uint64_t* b) {
    const uint64_t lo = *a < *b ? *a : *b, hi = *a < *b ? *b : *a;
    *a = lo; *b = hi;
}
// Eight words sorted ascending by Batcher's odd-even merge network: 19 compare-exchanges at fixed positions, so the words stay in registers.
PT_HD void matte_sort8(uint64_t (&v)[8]) {
#define PT_MATTE_CE(i, j) matte_compare_exchange(&v[i], &v[j])
    PT_MATTE_CE(0, 1); PT_MATTE_CE(2, 3); PT_MATTE_CE(4, 5); PT_MATTE_CE(6, 7);
    PT_MATTE_CE(0, 2); PT_MATTE_CE(1, 3); PT_MATTE_CE(4, 6); PT_MATTE_CE(5, 7);
    PT_MATTE_CE(1, 2); PT_MATTE_CE(5, 6);
    PT_MATTE_CE(0, 4); PT_MATTE_CE(1, 5); PT_MATTE_CE(2, 6); PT_MATTE_CE(3, 7);
    PT_MATTE_CE(2, 4); PT_MATTE_CE(3, 5);
    PT_MATTE_CE(1, 2); PT_MATTE_CE(3, 4); PT_MATTE_CE(5, 6);
#undef PT_MATTE_CE
}
// The finish of one pixel: R slots in, R ranked (key, coverage) pairs out.  Slots R .. 7 of the network are empty ones, which sort last.
template <int R>
PT_HD void matte_finish_pixel(const MatteSlot (&s)[R], uint32_t samples, uint32_t (&keys)[R], float (&coverage)[R]) {
    uint64_t v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = matte_order_word(r < R ? s[r < R ? r : 0] : MatteSlot{MATTE_NONE, 0u});
    matte_sort8(v);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t count = ~(uint32_t)(v[r] >> 32);
        keys[r] = (uint32_t)v[r];
        coverage[r] = count == 0u ? 0.0f : (float)count / (float)samples;
    }
}

// whether `key` is among selected[lo .. hi-1], sorted ascending without duplicates
PT_HD bool matte_in_set(const uint32_t* selected, uint32_t lo, uint32_t hi, uint32_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const uint32_t v = selected[mid];
        if (v == key) return true;
        if (v < key) lo = mid + 1u; else hi = mid;
    }
    return false;
}
// one pixel's coverage of the set selected[lo .. hi-1]
template <int R>
PT_HD float matte_extract_pixel(const uint32_t (&keys)[R], const float (&coverage)[R], const uint32_t* selected, uint32_t lo, uint32_t hi) {
    float out = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (keys[r] != MATTE_NONE && matte_in_set(selected, lo, hi, keys[r])) out = out + coverage[r];
    return out;
}

// MurmurHash3_x86_32 (Austin Appleby, public domain), written from its definition
PT_HD uint32_t matte_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
PT_HD uint32_t matte_murmur3_32(const uint8_t* data, size_t len, uint32_t seed) {
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h = seed;
    const size_t blocks = len / 4;
    for (size_t i = 0; i < blocks; ++i) {
        uint32_t k = (uint32_t)data[4 * i] | ((uint32_t)data[4 * i + 1] << 8) | ((uint32_t)data[4 * i + 2] << 16) | ((uint32_t)data[4 * i + 3] << 24);
        k *= c1; k = matte_rotl(k, 15); k *= c2;
        h ^= k; h = matte_rotl(h, 13); h = h * 5u + 0xe6546b64u;
    }
    const uint8_t* tail = data + 4 * blocks;
    uint32_t k = 0u;
    switch (len & 3u) {
        case 3: k ^= (uint32_t)tail[2] << 16;   // fallthrough
        case 2: k ^= (uint32_t)tail[1] << 8;    // fallthrough
        case 1: k ^= (uint32_t)tail[0];
                k *= c1; k = matte_rotl(k, 15); k *= c2; h ^= k;
    }
    h ^= (uint32_t)len;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
// the bits of the id float of a hash
PT_HD uint32_t matte_id_bits(uint32_t hash) {
    const uint32_t exponent = (hash >> 23) & 255u;
    return (exponent == 0u || exponent == 255u) ? hash ^ (1u << 23) : hash;
}

}  // namespace ptd
#endif
