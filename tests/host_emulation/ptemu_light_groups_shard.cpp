// ptemu_light_groups_shard.cpp — TEST HARNESS: the packed shard of the group node entries (include/pt_light_groups_multi.h, DESIGN.md section 15 "On every
// device of a node") on the CPU.  A library of its own beside pt_plan.cpp (tests/test_light_groups_multi.py builds it); not part of the product.
//
// Its entry points run the engine's own text over arrays the caller gives: pt_shard_rules.h (what k_light_groups_pack and k_light_groups_unpack do
// lane after lane, and the host scatter of the node entries), pth::shard_pixels, and the pth::check_* functions the node entries call before they look for a
// device.  The pixels are moved as ShardPixel, four floats at a float's alignment: what the engine's host threads move.
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_shard_rules.h"
#include "../../include/pt_light_groups_multi.h"

using namespace ptd;

static thread_local std::string g_shard_error;

extern "C" {

const char* ptemu_light_groups_shard_last_error(void) { return g_shard_error.c_str(); }

// pth::shard_pixels: the number of pixels of the shard; the list itself into px when it fits `capacity`
uint32_t ptemu_lg_shard_pixels(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t shard_index, uint32_t shard_count, uint32_t* px, uint32_t capacity) {
    const std::vector<uint32_t> list = pth::shard_pixels(width, height, tile_w, tile_h, shard_index, shard_count);
    if (px && list.size() <= capacity) for (size_t i = 0; i < list.size(); ++i) px[i] = list[i];
    return (uint32_t)list.size();
}

// one launch of k_light_groups_pack: every item of the list, in lane order
void ptemu_light_groups_shard_pack(const float* group_films, uint32_t film_pixels, const uint32_t* px, uint32_t n_own, uint32_t groups, float* packed) {
    for (uint32_t i = 0; i < n_own; ++i)
        shard_pack_item(reinterpret_cast<const ShardPixel*>(group_films), film_pixels, px, n_own, groups, i, reinterpret_cast<ShardPixel*>(packed));
}

// what a worker of the node entries does with its staging buffer (and, with groups = 1, what the node-resident mix does with a shard's mixed pixels)
void ptemu_light_groups_shard_scatter(const float* packed, const uint32_t* px, uint32_t n_own, uint32_t groups, float* group_films, uint32_t film_pixels) {
    shard_scatter(reinterpret_cast<const ShardPixel*>(packed), px, n_own, groups, reinterpret_cast<ShardPixel*>(group_films), film_pixels);
}

// one launch of k_light_groups_unpack (pt_resident_assemble): every item of the list, in lane order
void ptemu_light_groups_shard_unpack(const float* packed, const uint32_t* px, uint32_t n_own, uint32_t groups, float* group_films, uint32_t film_pixels) {
    for (uint32_t i = 0; i < n_own; ++i)
        shard_unpack_item(reinterpret_cast<const ShardPixel*>(packed), px, n_own, groups, i, reinterpret_cast<ShardPixel*>(group_films), film_pixels);
}

// the argument checks of pt_render_light_groups_multi and pt_render_adaptive_light_groups_multi (the scene is only compared with null)
pt_status ptemu_light_groups_multi_check(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, uint32_t camera_count,
                                         const void* film) {
    pt_render_desc out;
    return pth::check_light_groups_multi_args(scene, rd, gd, scene_instances, camera_count, film, &out, &g_shard_error);
}
pt_status ptemu_adaptive_light_groups_multi_check(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_light_groups_desc* gd,
                                                  uint32_t scene_instances, uint32_t camera_count, const void* film, const void* sample_counts) {
    pt_render_desc out;
    pt_adaptive_desc ad_out;
    return pth::check_adaptive_light_groups_multi_args(scene, rd, ad, gd, scene_instances, camera_count, film, sample_counts, &out, &ad_out, &g_shard_error);
}
// the one-device checks, for the comparison of the words
pt_status ptemu_light_groups_one_check(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, const void* film) {
    return pth::check_light_groups_args(scene, rd, gd, scene_instances, film, &g_shard_error);
}

}  // extern "C"
