// pt_light_groups_shard_rules.h — the index rule of a shard's packed group films (pt_render_light_groups_multi / pt_render_adaptive_light_groups_multi of
// include/pt_light_groups_multi.h, DESIGN.md section 15 "On every device of a node") as PT_HD functions that the pack and unpack kernels
// (pt_light_groups_shard.hip), the host scatter of the node entries (pt_engine.hip) and the host emulation of the tests
// (tests/host_emulation/ptemu_light_groups_shard.cpp) all compile: one text, so they agree.
//
// A device of a node call renders into full-size group films, films[g * film_pixels + pixel] in pixels of four floats, that are non-zero only on its own
// tiles.  With px the shard's pixel list in pth::shard_pixels' order (n_own entries) its packed films are
//     packed[g * n_own + i] = films[g * film_pixels + px[i]]        i = 0 .. n_own-1,  g = 0 .. G-1
// and the scatter is the same assignment read from right to left.  Pixels are moved, never computed with: every bit pattern survives, NaN payloads and
// -0.0 included.  Every pixel of a film is in exactly one shard's list (tests/test_light_groups_multi.py), so scattering every shard writes every pixel of
// every group film exactly once.  A mixed film (pt_light_groups_mix_resident over the shards) is scattered by the same rule with G = 1.
//
// Q is the pixel as the caller moves it: the kernels take HIP's float4, one 16-byte load and one 16-byte store; the host takes LgPixel, four floats at a
// float's alignment, because the caller's arrays promise no more.
#ifndef PT_LIGHT_GROUPS_SHARD_RULES_H
#define PT_LIGHT_GROUPS_SHARD_RULES_H
#include <stddef.h>

#include "../../include/pt_numerics.h"

namespace ptd {

struct LgPixel { float v[4]; };

PT_HD size_t lg_shard_packed_index(uint32_t g, uint32_t n_own, uint32_t i) { return (size_t)g * n_own + i; }
PT_HD size_t lg_shard_film_index(uint32_t g, size_t film_pixels, uint32_t pixel) { return (size_t)g * film_pixels + pixel; }

// Item i of a shard, every group: px[i] is read once
template <typename Q>
PT_HD void lg_shard_pack_item(const Q* films, size_t film_pixels, const uint32_t* px, uint32_t n_own, uint32_t groups, uint32_t i, Q* packed) {
    const uint32_t pixel = px[i];
#pragma unroll 4   // (four pixel loads in flight per lane)
    for (uint32_t g = 0; g < groups; ++g) packed[lg_shard_packed_index(g, n_own, i)] = films[lg_shard_film_index(g, film_pixels, pixel)];
}
// The inverse, item i of a shard, every group: px[i] is read once; item by item, so the destination films need no zeroing and the shards may be unpacked in
// any order
template <typename Q>
PT_HD void lg_shard_unpack_item(const Q* packed, const uint32_t* px, uint32_t n_own, uint32_t groups, uint32_t i, Q* films, size_t film_pixels) {
    const uint32_t pixel = px[i];
#pragma unroll 4   // (four packed loads in flight per lane)
    for (uint32_t g = 0; g < groups; ++g) films[lg_shard_film_index(g, film_pixels, pixel)] = packed[lg_shard_packed_index(g, n_own, i)];
}
// A whole shard back into full-size films, film by film: a host thread reads its packed films in order and writes runs of a tile row
template <typename Q>
PT_HD void lg_shard_scatter(const Q* packed, const uint32_t* px, uint32_t n_own, uint32_t groups, Q* films, size_t film_pixels) {
    for (uint32_t g = 0; g < groups; ++g)
        for (uint32_t i = 0; i < n_own; ++i) films[lg_shard_film_index(g, film_pixels, px[i])] = packed[lg_shard_packed_index(g, n_own, i)];
}

}  // namespace ptd
#endif
