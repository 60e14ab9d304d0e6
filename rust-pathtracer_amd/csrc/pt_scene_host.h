// pt_scene_host.h — host-side scene flattening for the HIP engine (see pt_scene_host.cpp).
#ifndef PT_SCENE_HOST_H
#define PT_SCENE_HOST_H
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_blob.h"

namespace pth {

struct HostScene {
    std::vector<uint32_t> blob;   // pt_blob.h layout
    std::vector<float> tex;       // texture texels
    std::vector<pt_camera> cameras;
    std::vector<uint32_t> curve_offsets;
    std::vector<int> mesh_has_light;
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

}  // namespace pth
#endif
