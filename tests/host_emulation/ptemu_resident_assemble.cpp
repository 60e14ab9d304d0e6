// ptemu_resident_assemble.cpp — TEST HARNESS: what pt_resident_assemble (include/pt_resident.h, DESIGN.md section 14, "Assembling a node render") rests on, on the
// CPU.  Linked into a library of its own beside ptemu_spectral_shard.cpp and pt_plan.cpp (tests/test_resident_assemble.py builds it); not part of the product.
//
// Its entry points run the engine's own text: shard_unpack_item of pt_shard_rules.h, what k_spectral_unpack does lane after lane, over arrays
// the caller gives, and pth::check_resident_assemble, which the entry runs before it looks for a device, over a remembered node render given as plain arguments.
#include <string>

#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_shard_rules.h"
#include "../../include/pt_resident.h"

using namespace ptd;

static thread_local std::string g_assemble_error;

extern "C" {

const char* ptemu_resident_assemble_last_error(void) { return g_assemble_error.c_str(); }

// one launch of k_spectral_unpack: every item of the list, in lane order
void ptemu_spectral_shard_unpack(const float* packed, const uint32_t* px, uint32_t n_own, uint32_t bins, float* planes, uint32_t plane_pixels) {
    for (uint32_t i = 0; i < n_own; ++i) shard_unpack_item(packed, px, n_own, bins, i, planes, plane_pixels);
}

// the checks of pt_resident_assemble (the scene is only compared with null); remembered: whether the scene holds the description of a node render at all
pt_status ptemu_resident_assemble_check(const void* scene, uint32_t flags, int remembered, int with_stats, uint32_t width, uint32_t height, uint32_t bins) {
    pth::NodeRender node;
    node.valid = remembered != 0; node.stats = with_stats != 0;
    node.width = width; node.height = height; node.bins = bins;
    return pth::check_resident_assemble(scene, flags, node, &g_assemble_error);
}

}  // extern "C"
