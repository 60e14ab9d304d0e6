// pt_scene_host.h — host-side scene flattening for the HIP engine (see pt_scene_host.cpp).
#ifndef PT_SCENE_HOST_H
#define PT_SCENE_HOST_H
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pt_api.h"
#include "../../include/pt_light_groups_spectral.h"
#include "pt_blob.h"

namespace pth {

struct HostScene {
    std::vector<uint32_t> blob;   // pt_blob.h layout
    std::vector<float> tex;       // texture texels
    std::vector<pt_camera> cameras;
    std::vector<uint32_t> curve_offsets;
    uint32_t light_count = 0, material_count = 0, curve_count = 0;
};

bool build_host_scene(const pt_scene_desc& desc, HostScene* out, std::string* error);

// A blob that holds nothing but curve records (behind an empty header), by the text that flattens a scene's curves: blob->data() is a SceneView's core
// section for ptd::curve_eval at the word offsets *curve_offsets.  curve_data holds curve_data_count floats.
bool build_curve_view(const pt_curve* curves, uint32_t curve_count, const float* curve_data, size_t curve_data_count, std::vector<uint32_t>* blob,
                      std::vector<uint32_t>* curve_offsets, std::string* error);

// pt_spectral_response_matrix (include/pt_spectral.h) behind its argument check (pth::check_response_matrix_args): the lane code of
// pt_spectral_project_rules.h on the host over build_curve_view's blob.  matrix: K * bins floats.
bool spectral_response_matrix(float wavelength_lo, float wavelength_hi, uint32_t bins, const pt_curve* curves, uint32_t curve_count, const float* curve_data,
                              size_t curve_data_count, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, float* matrix, std::string* error);

// include/pt_light_groups_spectral.h, for the engine and the host emulation alike.  check_light_groups_spectral_args: pth::check_light_groups_args, the spectral
// desc and the film's size.  check_relamp_matrix: K, G, bins in range and every entry finite (the resident entry checks against its resident bins);
// check_relamp_args: the host-array entry's.  light_groups_relamp_matrix: pt_light_groups_relamp_matrix whole — its refusals, then the lane code of
// pt_light_groups_spectral_rules.h on the host over build_curve_view's blob.  matrix: K * group_count * bins floats.
pt_status check_light_groups_spectral_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, const pt_spectral_desc* sd, uint32_t scene_instances,
                                           const void* film, std::string* error);
pt_status check_relamp_matrix(uint32_t K, uint32_t group_count, uint32_t bins, const float* matrix, std::string* error);
pt_status check_relamp_args(uint32_t width, uint32_t height, uint32_t group_count, uint32_t bins, uint32_t K, const float* matrix, const void* group_spectral,
                            const void* out, std::string* error);
pt_status light_groups_relamp_matrix(const pt_render_desc* rd, const pt_spectral_desc* sd, const pt_curve* curves, uint32_t curve_count, const float* curve_data,
                                     uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, uint32_t group_count,
                                     const int32_t* old_curve, const int32_t* new_curve, const float* gain, float* matrix, std::string* error);

}  // namespace pth
#endif
