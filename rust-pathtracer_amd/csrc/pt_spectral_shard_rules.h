// pt_spectral_shard_rules.h — the index rule of a shard's packed spectral film (pt_render_spectral_multi / pt_render_adaptive_spectral_multi of
// include/pt_spectral.h) as PT_HD functions that the pack kernel (pt_spectral_shard.hip), the host scatter of the node entries
// (pt_engine.hip) and the host emulation of the tests (tests/host_emulation/ptemu_spectral_shard.cpp) all compile: one text, so they agree.
//
// A device of a node call renders into full-size planes, planes[b * plane_pixels + pixel], that are non-zero only on its own tiles.  With px the shard's
// pixel list in pth::shard_pixels' order (n_own entries) its packed film is
//     packed[b * n_own + i] = planes[b * plane_pixels + px[i]]        i = 0 .. n_own-1,  b = 0 .. bins-1
// and the scatter is the same assignment read from right to left.  Values are moved, never computed with: every bit pattern survives, NaN payloads and
// -0.0 included.  Every pixel of a film is in exactly one shard's list (tests/test_spectral_multi.py), so scattering every shard writes every float of
// the planes exactly once.  The planes of a development (K of them, pt_spectral_project_resident) are scattered by the same rule with bins = K.
// spectral_shard_unpack_item is the scatter as the device runs it (k_spectral_unpack, pt_resident_assemble of include/pt_resident.h): item by item, so the
// destination planes need no zeroing and the shards may be unpacked in any order or side by side.
#ifndef PT_SPECTRAL_SHARD_RULES_H
#define PT_SPECTRAL_SHARD_RULES_H
#include <stddef.h>

#include "../../include/pt_numerics.h"

namespace ptd {

PT_HD size_t spectral_shard_packed_index(uint32_t b, uint32_t n_own, uint32_t i) { return (size_t)b * n_own + i; }
PT_HD size_t spectral_shard_plane_index(uint32_t b, size_t plane_pixels, uint32_t pixel) { return (size_t)b * plane_pixels + pixel; }

// Item i of a shard, every bin: px[i] is read once
PT_HD void spectral_shard_pack_item(const float* planes, size_t plane_pixels, const uint32_t* px, uint32_t n_own, uint32_t bins, uint32_t i, float* packed) {
    const uint32_t pixel = px[i];
#pragma unroll 4   // (four plane loads in flight per lane)
    for (uint32_t b = 0; b < bins; ++b) packed[spectral_shard_packed_index(b, n_own, i)] = planes[spectral_shard_plane_index(b, plane_pixels, pixel)];
}
// The inverse, item i of a shard, every bin: px[i] is read once
PT_HD void spectral_shard_unpack_item(const float* packed, const uint32_t* px, uint32_t n_own, uint32_t bins, uint32_t i, float* planes, size_t plane_pixels) {
    const uint32_t pixel = px[i];
#pragma unroll 4   // (four packed loads in flight per lane)
    for (uint32_t b = 0; b < bins; ++b) planes[spectral_shard_plane_index(b, plane_pixels, pixel)] = packed[spectral_shard_packed_index(b, n_own, i)];
}
// A whole shard back into full-size planes, plane by plane: a host thread reads its packed planes in order and writes runs of a tile row
PT_HD void spectral_shard_scatter(const float* packed, const uint32_t* px, uint32_t n_own, uint32_t bins, float* planes, size_t plane_pixels) {
    for (uint32_t b = 0; b < bins; ++b)
        for (uint32_t i = 0; i < n_own; ++i) planes[spectral_shard_plane_index(b, plane_pixels, px[i])] = packed[spectral_shard_packed_index(b, n_own, i)];
}

}  // namespace ptd
#endif
