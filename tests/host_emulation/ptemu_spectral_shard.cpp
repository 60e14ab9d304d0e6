// ptemu_spectral_shard.cpp — TEST HARNESS: the packed shard of the spectral node entries (include/pt_spectral.h) on the CPU.  A library
// of its own beside pt_plan.cpp (tests/test_spectral_multi.py builds it); not part of the product.
//
// Its entry points run the engine's own text over arrays the caller gives: pt_shard_rules.h (what k_spectral_pack does lane after lane, and the host
// scatter of the node entries), pth::shard_pixels, and the pth::check_* functions the node entries call before they look for a device.
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_shard_rules.h"
#include "../../include/pt_spectral.h"

using namespace ptd;

static thread_local std::string g_shard_error;

extern "C" {

const char* ptemu_spectral_shard_last_error(void) { return g_shard_error.c_str(); }

// pth::shard_pixels: the number of pixels of the shard; the list itself into px when it fits `capacity`
uint32_t ptemu_shard_pixels(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t shard_index, uint32_t shard_count, uint32_t* px, uint32_t capacity) {
    const std::vector<uint32_t> list = pth::shard_pixels(width, height, tile_w, tile_h, shard_index, shard_count);
    if (px && list.size() <= capacity) for (size_t i = 0; i < list.size(); ++i) px[i] = list[i];
    return (uint32_t)list.size();
}

// one launch of k_spectral_pack: every item of the list, in lane order
void ptemu_spectral_shard_pack(const float* planes, uint32_t plane_pixels, const uint32_t* px, uint32_t n_own, uint32_t bins, float* packed) {
    for (uint32_t i = 0; i < n_own; ++i) shard_pack_item(planes, plane_pixels, px, n_own, bins, i, packed);
}

// what a worker of the node entries does with its staging buffer
void ptemu_spectral_shard_scatter(const float* packed, const uint32_t* px, uint32_t n_own, uint32_t bins, float* planes, uint32_t plane_pixels) {
    shard_scatter(packed, px, n_own, bins, planes, plane_pixels);
}

// the argument checks of pt_render_spectral_multi and pt_render_adaptive_spectral_multi (the scene is only compared with null)
pt_status ptemu_spectral_multi_check(const void* scene, const pt_render_desc* rd, const pt_spectral_desc* sd, uint32_t camera_count, const void* film, const void* spectral) {
    pt_render_desc out;
    return pth::check_spectral_multi_args(scene, rd, sd, camera_count, film, spectral, &out, &g_shard_error);
}
pt_status ptemu_adaptive_spectral_multi_check(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_spectral_desc* sd, uint32_t camera_count,
                                              const void* film, const void* sample_counts, const void* spectral) {
    pt_render_desc out;
    pt_adaptive_desc ad_out;
    return pth::check_adaptive_spectral_args(scene, rd, ad, sd, camera_count, film, sample_counts, spectral, &out, &ad_out, &g_shard_error);
}

}  // extern "C"
