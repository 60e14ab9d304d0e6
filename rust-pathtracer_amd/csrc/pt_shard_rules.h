// pt_shard_rules.h — the index rule of a shard's packed planes: the spectral film of pt_render_spectral_multi / pt_render_adaptive_spectral_multi
// (include/pt_spectral.h) and the group films of pt_render_light_groups_multi / pt_render_adaptive_light_groups_multi
// (include/pt_light_groups_multi.h, DESIGN.md section 15 "On every device of a node"), as PT_HD functions that the pack and unpack kernels (pt_shard.hip), the
// host scatter of the node entries (pt_engine.hip) and the host emulation of the tests (tests/host_emulation/ptemu_spectral_shard.cpp,
// ptemu_resident_assemble.cpp, ptemu_light_groups_shard.cpp) all compile: one text, so they agree.
//
// A device of a node call renders into full-size planes, full[p * full_pixels + pixel], that are non-zero only on its own tiles: the bins of a spectral film
// in floats, the group films in pixels of four floats.  With px the shard's pixel list in pth::shard_pixels' order (n_own entries) its packed planes are
//     packed[p * n_own + i] = full[p * full_pixels + px[i]]        i = 0 .. n_own-1,  p = 0 .. planes-1
// and the scatter is the same assignment read from right to left.  Elements are moved, never computed with: every bit pattern survives, NaN payloads and
// -0.0 included.  Every pixel of a film is in exactly one shard's list (tests/test_spectral_multi.py, tests/test_light_groups_multi.py), so scattering every
// shard writes every element of the planes exactly once.  The planes of a development (K of them, pt_spectral_project_resident) and a mixed film (one plane of
// pixels, pt_light_groups_mix_resident) are scattered by the same rule.
//
// Q is the element as the caller moves it: float for the bins and the planes of a development; for the group films and a mixed film the 16-byte pixel — the
// kernels take HIP's float4, one 16-byte load and one 16-byte store; the host takes ShardPixel, four floats at a float's alignment, because the caller's
// arrays promise no more.
#ifndef PT_SHARD_RULES_H
#define PT_SHARD_RULES_H
#include <stddef.h>

#include "../../include/pt_numerics.h"

namespace ptd {

struct ShardPixel { float v[4]; };

PT_HD size_t shard_packed_index(uint32_t p, uint32_t n_own, uint32_t i) { return (size_t)p * n_own + i; }
PT_HD size_t shard_full_index(uint32_t p, size_t full_pixels, uint32_t pixel) { return (size_t)p * full_pixels + pixel; }

// Item i of a shard, every plane: px[i] is read once
template <typename Q>
PT_HD void shard_pack_item(const Q* full, size_t full_pixels, const uint32_t* px, uint32_t n_own, uint32_t planes, uint32_t i, Q* packed) {
    const uint32_t pixel = px[i];
#pragma unroll 4   // (four plane loads in flight per lane)
    for (uint32_t p = 0; p < planes; ++p) packed[shard_packed_index(p, n_own, i)] = full[shard_full_index(p, full_pixels, pixel)];
}
// The inverse, item i of a shard, every plane: px[i] is read once.  The scatter as the device runs it (pt_resident_assemble of include/pt_resident.h): item by
// item, so the destination planes need no zeroing and the shards may be unpacked in any order or side by side
template <typename Q>
PT_HD void shard_unpack_item(const Q* packed, const uint32_t* px, uint32_t n_own, uint32_t planes, uint32_t i, Q* full, size_t full_pixels) {
    const uint32_t pixel = px[i];
#pragma unroll 4   // (four packed loads in flight per lane)
    for (uint32_t p = 0; p < planes; ++p) full[shard_full_index(p, full_pixels, pixel)] = packed[shard_packed_index(p, n_own, i)];
}
// A whole shard back into full-size planes, plane by plane: a host thread reads its packed planes in order and writes runs of a tile row
template <typename Q>
PT_HD void shard_scatter(const Q* packed, const uint32_t* px, uint32_t n_own, uint32_t planes, Q* full, size_t full_pixels) {
    for (uint32_t p = 0; p < planes; ++p)
        for (uint32_t i = 0; i < n_own; ++i) full[shard_full_index(p, full_pixels, px[i])] = packed[shard_packed_index(p, n_own, i)];
}

}  // namespace ptd
#endif
