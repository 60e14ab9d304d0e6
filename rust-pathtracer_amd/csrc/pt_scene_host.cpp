// pt_scene_host.cpp — host side of pt_scene_create: validates a pt_scene_desc, builds the two BVH levels and
// packs everything into the word blob of pt_blob.h.  Runs once per scene, outside the timed render loop
// (the reference's equivalent work is construct_world + Mesh::init + Accelerator::new,
// src/parsing/mod.rs:145-563, src/geometry/mesh.rs:283-305, src/accelerator/mod.rs:31-43).
// The build is SceneBuild::run, a list of stages in the order of the blob's layout; what it makes is pinned word for word by tests/test_scene_blob.py.
// pt_scene_bvh.h (the box and the BVH builder) and pt_scene_certify.h (closed, convex, inner balls) are this file's alone.
#include "pt_scene_host.h"
#include "pt_device.h"
#include "pt_spectral_project_rules.h"
#include "pt_light_groups_spectral_rules.h"
#include "pt_plan.h"
#include "pt_scene_bvh.h"
#include "pt_scene_certify.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pth {

namespace {

void pad16(std::vector<uint32_t>& w) { while (w.size() % 4) w.push_back(0); }

void xf_point(const float* m, const float* p, float* o) {
    for (int r = 0; r < 3; ++r) o[r] = m[4 * r] * p[0] + m[4 * r + 1] * p[1] + m[4 * r + 2] * p[2] + m[4 * r + 3];
}

// Matrix4x4 * AABB (aabb.rs:116-138): the box of the eight transformed corners
Box transformed_box(const Box& b, const float* forward) {
    Box t = box_empty();
    for (int c = 0; c < 8; ++c) {
        float p[3] = {(c & 1) == 0 ? b.mn[0] : b.mx[0], ((c >> 1) & 1) == 0 ? b.mn[1] : b.mx[1], ((c >> 2) & 1) == 0 ? b.mn[2] : b.mx[2]}, q[3];
        xf_point(forward, p, q); box_grow(t, q);
    }
    return t;
}

// The object-space box of an analytic shape.  `disk_extent`: how far a disk's box reaches from its origin in x and y — the reference's is half the radius
// (disk.rs:23-28, a quirk kept in the tree), the disk's own is the radius (what a certificate must clear).
Box shape_box(const pt_instance& in, float disk_extent) {
    float v[3] = {in.radius, in.radius, in.radius};   // sphere.rs:24-31
    if (in.kind == PT_SHAPE_RECT) {  // rect.rs:58-66
        float hx = in.size[0] / 2.0f, hy = in.size[1] / 2.0f;
        if (in.axis == PT_AXIS_X) { v[0] = 0.0001f; v[1] = hy; v[2] = hx; }
        else if (in.axis == PT_AXIS_Y) { v[0] = hx; v[1] = 0.0001f; v[2] = hy; }
        else { v[0] = hx; v[1] = hy; v[2] = 0.0001f; }
    } else if (in.kind == PT_SHAPE_DISK) { v[0] = disk_extent; v[1] = disk_extent; v[2] = 0.001f; }
    float lo[3], hi[3]; for (int k = 0; k < 3; ++k) { lo[k] = in.origin[k] - v[k]; hi[k] = in.origin[k] + v[k]; }
    return box_of_corners(lo, hi);
}

// BOUNDED_VISIBLE_RANGE in 100 left-Riemann steps, as Curve::evaluate_integral walks it: sum of f(k) * step, f(k) taken at visible_lambda(k)
const int kVisibleSteps = 100;
const float kVisibleStep = (750.0f - 380.0f) / 100.0f;
float visible_lambda(int k) { return 380.0f + (float)k * kVisibleStep; }
template <class F> float visible_range_sum(F f) {
    float sum = 0.0f;
    for (int k = 0; k < kVisibleSteps; ++k) sum += f(k) * kVisibleStep;
    return sum;
}

// MeshTriangleRef::surface_area (mesh.rs:200-210) in object space, f32, in its order: Heron's formula over the edge lengths |p2 - p0|, |p1 - p0|, |p2 - p1|
// (a length: sqrt(x x + y y + z z), left to right).  A degenerate face can give 0 or NaN: its sample's pdf is then not finite and becomes 0 (light_sample).
float triangle_area(const float* V, const uint32_t* ix) {
    auto dist = [&](uint32_t a, uint32_t b) {
        const float x = V[3 * b] - V[3 * a], y = V[3 * b + 1] - V[3 * a + 1], z = V[3 * b + 2] - V[3 * a + 2];
        return std::sqrt(x * x + y * y + z * z);
    };
    const float d02 = dist(ix[0], ix[2]), d01 = dist(ix[0], ix[1]), d12 = dist(ix[1], ix[2]);
    const float s = 0.5f * (d02 + d01 + d12);
    return std::sqrt(s * (s - d01) * (s - d12) * (s - d02));
}

}  // namespace

// The curves' validation and their records in the blob, for build_host_scene and for build_curve_view alike (one text: a curve's value is the same in both).
static const char* check_curves(const pt_curve* curves, uint32_t curve_count, size_t curve_data_count) {
    for (uint32_t i = 0; i < curve_count; ++i) {
        const pt_curve& c = curves[i];
        uint32_t per = c.kind == PT_CURVE_TABULATED ? 2 : ((c.kind == PT_CURVE_EXPONENTIAL || c.kind == PT_CURVE_INV_EXPONENTIAL) ? 4 : 1);
        bool needs_data = c.kind == PT_CURVE_LINEAR || c.kind == PT_CURVE_TABULATED || c.kind == PT_CURVE_EXPONENTIAL || c.kind == PT_CURVE_INV_EXPONENTIAL;
        if (c.kind < 0 || c.kind > PT_CURVE_CONST) return "unknown curve kind";
        if (needs_data && ((size_t)c.data_offset + (size_t)c.data_count * per > curve_data_count)) return "curve data out of range";
        if ((c.kind == PT_CURVE_LINEAR || c.kind == PT_CURVE_TABULATED) && c.data_count == 0) return "empty curve table";
    }
    return nullptr;
}
static void flatten_curves(const pt_curve* curves, uint32_t curve_count, const float* curve_data, bool curve_tables, std::vector<uint32_t>& w,
                           std::vector<uint32_t>* curve_off_out, uint32_t* curve_table_words) {
    pad16(w);
    std::vector<uint32_t>& curve_off = *curve_off_out;
    curve_off.assign(curve_count, 0);
    for (uint32_t i = 0; i < curve_count; ++i) { curve_off[i] = (uint32_t)w.size(); w.resize(w.size() + PT_CURVE_WORDS, 0); }
    for (uint32_t i = 0; i < curve_count; ++i) {
        const pt_curve& c = curves[i];
        uint32_t per = c.kind == PT_CURVE_TABULATED ? 2 : ((c.kind == PT_CURVE_EXPONENTIAL || c.kind == PT_CURVE_INV_EXPONENTIAL) ? 4 : 1);
        uint32_t off = (uint32_t)w.size();
        bool has = c.kind == PT_CURVE_LINEAR || c.kind == PT_CURVE_TABULATED || c.kind == PT_CURVE_EXPONENTIAL || c.kind == PT_CURVE_INV_EXPONENTIAL;
        if (has) for (uint32_t k = 0; k < c.data_count * per; ++k) w.push_back(fbits(curve_data[c.data_offset + k]));
        // A tabulated curve's cell table (round 5; pt_blob.h PT_CURVE_GRID): the knot range in G equal cells, per cell the number of knots in lower cells — a lower
        // bound of the binary search's answer for every wavelength of the cell (cell() is monotone), from which curve_eval walks up: the same index, one or two knot
        // reads instead of log2 n.  cell() here is curve_grid_cell's arithmetic (pt_device.h), operation for operation.
        uint32_t grid_word = 0, inv_bits = 0;
        if (curve_tables && c.kind == PT_CURVE_TABULATED && c.data_count >= PT_CURVE_GRID_MIN_KNOTS && c.data_count <= 255u) {
            const float* kd = curve_data + c.data_offset;
            const uint32_t n = c.data_count;
            bool sorted = true;
            for (uint32_t k = 0; k < n; ++k) sorted = sorted && std::isfinite(kd[2 * k]) && (k == 0 || kd[2 * k] >= kd[2 * (k - 1)]);
            uint32_t cells = 16; while (cells < n) cells *= 2;
            const float x0 = kd[0], width = kd[2 * (n - 1)] - x0;
            const float inv = (float)cells / width;
            if (sorted && width > 0.0f && std::isfinite(inv) && inv > 0.0f && w.size() < (1u << 24)) {   // (the table's word offset rides in 24 bits of the record's grid word: a core section beyond 64 MB keeps the binary search)
                const float top = (float)(cells - 1);
                std::vector<uint32_t> below(cells + 1, 0);   // below[g] = knots in cells < g
                for (uint32_t k = 0; k < n; ++k) {
                    const float fi = (kd[2 * k] - x0) * inv;
                    const uint32_t g = fi >= 0.0f ? (uint32_t)(fi < top ? fi : top) : 0u;
                    below[g + 1] += 1;
                }
                for (uint32_t g = 0; g < cells; ++g) below[g + 1] += below[g];
                const uint32_t toff = (uint32_t)w.size();
                for (uint32_t g = 0; g < cells; g += 4) w.push_back(below[g] | below[g + 1] << 8 | below[g + 2] << 16 | below[g + 3] << 24);
                grid_word = toff | (cells - 1) << 24; inv_bits = fbits(inv); *curve_table_words += cells / 4;
            }
        }
        uint32_t* r = &w[curve_off[i]];
        r[0] = (uint32_t)c.kind; r[1] = (uint32_t)c.mode; r[2] = fbits(c.p0); r[3] = fbits(c.p1); r[4] = off; r[5] = has ? c.data_count : 0;
        r[PT_CURVE_GRID] = grid_word; r[PT_CURVE_GRID_INV] = inv_bits;
    }
}
bool build_curve_view(const pt_curve* curves, uint32_t curve_count, const float* curve_data, size_t curve_data_count, std::vector<uint32_t>* blob,
                      std::vector<uint32_t>* curve_offsets, std::string* err) {
    if (const char* bad = check_curves(curves, curve_count, curve_data_count)) { *err = bad; return false; }
    blob->assign(PT_HDR_WORDS, 0);
    uint32_t table_words = 0;
    flatten_curves(curves, curve_count, curve_data, true, *blob, curve_offsets, &table_words);
    return true;
}

bool spectral_response_matrix(float lo, float hi, uint32_t bins, const pt_curve* curves, uint32_t curve_count, const float* curve_data, size_t curve_data_count,
                              uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, float* matrix, std::string* err) {
    std::vector<uint32_t> blob, off;
    if (!build_curve_view(curves, curve_count, curve_data, curve_data_count, &blob, &off, err)) return false;
    const float tex = 0.0f;
    ptd::SceneView view{blob.data(), &tex};
    const float w = (hi - lo) / (float)bins;
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t b = 0; b < bins; ++b) matrix[(size_t)k * bins + b] = ptd::spectral_matrix_entry(view, off.data(), responses[k], filter, lo, w, b, subsamples);
    return true;
}

// ---- include/pt_light_groups_spectral.h: the argument checks of its entries, for the engine and the host emulation alike
pt_status check_light_groups_spectral_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, const pt_spectral_desc* sd, uint32_t scene_instances,
                                           const void* film, std::string* error) {
    pt_status st = check_light_groups_args(scene, rd, gd, scene_instances, film, error);
    if (st != PT_OK) return st;
    st = check_spectral_desc(sd, error);
    if (st != PT_OK) return st;
    if (rd->width == 0 || rd->height == 0 || (uint64_t)rd->width * rd->height > 0x7fffffffull) {
        *error = "width and height must be positive and width x height must fit 31 bits";
        return PT_ERR_INVALID_ARGUMENT;
    }
    return PT_OK;
}

pt_status check_relamp_matrix(uint32_t K, uint32_t group_count, uint32_t bins, const float* matrix, std::string* error) {
    if (!matrix) { *error = "the re-lamp matrix is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (K == 0) { *error = "K must be positive: a re-lamp needs a response"; return PT_ERR_INVALID_ARGUMENT; }
    if (K > PT_SPECTRAL_MAX_RESPONSES) { *error = "K: at most 16 responses"; return PT_ERR_INVALID_ARGUMENT; }
    if (group_count == 0 || group_count > PT_LIGHT_GROUPS_MAX) { *error = "group_count must be in 1..8"; return PT_ERR_INVALID_ARGUMENT; }
    if (bins == 0) { *error = "bins must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (bins > PT_SPECTRAL_MAX_BINS) { *error = "bins: at most 64"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t i = 0; i < K * group_count * bins; ++i)
        if (!std::isfinite(matrix[i])) { *error = "re-lamp matrix entry " + std::to_string(i) + " is not finite"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_relamp_args(uint32_t width, uint32_t height, uint32_t group_count, uint32_t bins, uint32_t K, const float* matrix, const void* group_spectral,
                            const void* out, std::string* error) {
    if (!group_spectral) { *error = "the group bins are null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!out) { *error = "the re-lamped planes (out) are null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_relamp_matrix(K, group_count, bins, matrix, error);
    if (st != PT_OK) return st;
    if (width == 0 || height == 0) { *error = "width and height must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) { *error = "width x height must fit 31 bits"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

// pt_light_groups_relamp_matrix: pt_spectral_response_matrix's checks, then the groups' own, then the lane code of pt_light_groups_spectral_rules.h on the host
pt_status light_groups_relamp_matrix(const pt_render_desc* rd, const pt_spectral_desc* sd, const pt_curve* curves, uint32_t curve_count, const float* curve_data,
                                     uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, uint32_t group_count,
                                     const int32_t* old_curve, const int32_t* new_curve, const float* gain, float* matrix, std::string* error) {
    const pt_status st = check_response_matrix_args(rd, sd, curves, curve_count, curve_data, curve_data_floats, K, responses, filter, subsamples, matrix, error);
    if (st != PT_OK) return st;
    if (group_count == 0 || group_count > PT_LIGHT_GROUPS_MAX) { *error = "group_count must be in 1..8"; return PT_ERR_INVALID_ARGUMENT; }
    if (!old_curve || !new_curve) { *error = "old_curve or new_curve is null"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t g = 0; g < group_count; ++g) {
        const int32_t o = old_curve[g], n = new_curve[g];
        if (o != PT_RELAMP_KEEP && (o < 0 || (uint32_t)o >= curve_count)) {
            *error = "old_curve of group " + std::to_string(g) + " is neither a curve index nor PT_RELAMP_KEEP";
            return PT_ERR_INVALID_ARGUMENT;
        }
        if (n != PT_RELAMP_KEEP && (n < 0 || (uint32_t)n >= curve_count)) {
            *error = "new_curve of group " + std::to_string(g) + " is neither a curve index nor PT_RELAMP_KEEP";
            return PT_ERR_INVALID_ARGUMENT;
        }
        if (n == PT_RELAMP_KEEP && o != PT_RELAMP_KEEP) {
            *error = "group " + std::to_string(g) + " names an old curve and keeps its lamp: new_curve is PT_RELAMP_KEEP where old_curve is not";
            return PT_ERR_INVALID_ARGUMENT;
        }
        if (gain && !std::isfinite(gain[g])) { *error = "the gain of group " + std::to_string(g) + " is not finite"; return PT_ERR_INVALID_ARGUMENT; }
    }
    std::vector<uint32_t> blob, off;
    if (!build_curve_view(curves, curve_count, curve_data, curve_data_floats, &blob, &off, error)) return PT_ERR_INVALID_ARGUMENT;
    const float tex = 0.0f;
    ptd::SceneView view{blob.data(), &tex};
    const uint32_t bins = sd->bins;
    const float w = (rd->wavelength_hi - rd->wavelength_lo) / (float)bins;
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t g = 0; g < group_count; ++g) {
            const int32_t o = old_curve[g], n = o == PT_RELAMP_KEEP ? PT_RELAMP_KEEP : new_curve[g];   // (a kept group's new_curve is not looked at)
            for (uint32_t b = 0; b < bins; ++b) {
                const float m = ptd::lg_relamp_matrix_entry(view, off.data(), responses[k], filter, o, n, rd->wavelength_lo, w, b, subsamples);
                const float v = gain ? gain[g] * m : m;
                if (!std::isfinite(v)) {
                    *error = "the re-lamp matrix is not finite at response " + std::to_string(k) + ", group " + std::to_string(g) + ", bin " + std::to_string(b);
                    return PT_ERR_INVALID_ARGUMENT;
                }
                matrix[((size_t)k * group_count + g) * bins + b] = v;
            }
        }
    return PT_OK;
}

namespace {

// Records of `stride` words at w[base + k * stride], k < keys.size(), in any order of their own (the masks carry the leaf order): stable-sorted by key — the form
// of their box test, so that the sweep runs one loop per form — and copied into place; the bit table's box references (word 2 of a bit) that point into them
// follow.  Returns how many records carry each key (0..5).
std::array<uint32_t, 6> regroup_records(std::vector<uint32_t>& w, uint32_t base, uint32_t stride, const std::vector<uint32_t>& keys, std::vector<uint32_t>& bits) {
    std::vector<size_t> order(keys.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    std::vector<uint32_t> block(keys.size() * stride);
    std::vector<uint32_t> moved(keys.size());   // old record k -> its new word offset
    std::array<uint32_t, 6> counts = {0, 0, 0, 0, 0, 0};
    for (size_t pos = 0; pos < order.size(); ++pos) {
        const size_t k = order[pos];
        for (uint32_t q = 0; q < stride; ++q) block[pos * stride + q] = w[base + k * stride + q];
        moved[k] = base + (uint32_t)pos * stride;
        counts[keys[k]] += 1;
    }
    for (size_t b = 0; b < bits.size() / PT_SWEEP_BIT_WORDS; ++b) {
        uint32_t& bw = bits[b * PT_SWEEP_BIT_WORDS + 2];
        if (bw >= base && bw < base + keys.size() * stride) bw = moved[(bw - base) / stride] + (bw - base) % stride;
    }
    for (size_t q = 0; q < block.size(); ++q) w[base + q] = block[q];
    return counts;
}

// What the later stages need of a mesh once its data stands in the blob
struct MeshBuilt {
    Box box;                                      // Mesh::new bounding box over all vertices
    uint32_t node_off = 0, node_count = 0;        // its BVH, in the mesh section
    uint32_t tri_off = 0, perm0 = 0, perm1 = 0;   // its triangle records, and their two permuted copies relative to them (0 = none)
    uint32_t record = 0;                          // word offset of its record in the core section
    std::vector<uint32_t> light_faces;            // its emissive faces, in face order (one light-list entry each per instance)
    std::vector<uint32_t> face_flags;             // PT_TRI_FLAGS per face, merged over its certified instances (empty = none certified)
};

// One mesh on its way into the mesh section
struct MeshWork {
    const pt_mesh& m;
    const float* V;        // its vertices
    const uint32_t* ix;    // its faces' vertex indices
    MeshBuilt& out;
    std::vector<uint32_t> nodes;
    uint32_t normal_off = 0, leaf_off = 0, leaf_count = 0, group_off = 0;
};

// The leaf sweep table while it is made
struct SweepTable {
    uint32_t off = 0;             // word offset of the instance records
    std::vector<uint32_t> bits;   // PT_SWEEP_BIT_WORDS per mask bit
    std::vector<int> root_of;     // per bit: the bit whose box test it copies (itself if none)
    uint32_t bit = 0;             // the next free bit
    uint64_t mesh_mask = 0, owner_mask = 0;
    bool any_walked = false;
};

// The scene build: run() is the list of stages; each stage appends to the core words `w`, the mesh section `md` or the texels, in the order that is the blob's layout.
struct SceneBuild {
    const pt_scene_desc& d;
    HostScene* hs;
    std::string* err;
    std::vector<uint32_t>& w;                         // the core section (hs->blob; the mesh section joins it at the end)
    std::vector<uint32_t> md{0u, 0u, 0u, 0u};         // the mesh section: BVH nodes, triangles, normals, leaf lists; offsets relative to it (SceneView::m), so that
                                                      // the core alone can be staged in LDS when the whole scene does not fit
    std::vector<uint32_t> curve_off, ts_off;          // word offsets of the curve records and the texstacks
    std::vector<MeshBuilt> meshes;
    std::vector<Box> ibox;                            // the instances' world boxes
    std::vector<uint32_t> lights, light_faces;        // the light list; per entry the triangle word offset of the emissive face it stands for, 0 = an analytic light
    std::vector<uint32_t> top_nodes;                  // the top-level BVH
    const bool verbose = getenv("PT_AMD_HOST_VERBOSE") != nullptr;

    SceneBuild(const pt_scene_desc& desc, HostScene* out, std::string* error) : d(desc), hs(out), err(error), w(out->blob) {}

    bool fail(const char* m) { *err = m; return false; }
    bool curve_ok(int32_t c) const { return c >= 0 && (uint32_t)c < d.curve_count; }
    bool material_ok(uint32_t id) const { return id == PT_MATERIAL_NONE || PT_MATERIAL_INDEX(id) < d.material_count; }

    bool run(bool curve_tables, uint32_t* curve_table_words) {
        *curve_table_words = 0;
        if (!check_description()) return false;
        begin(curve_tables, curve_table_words);
        add_texstacks();
        add_materials();
        add_mediums();
        meshes.resize(d.mesh_count);
        for (uint32_t mi = 0; mi < d.mesh_count; ++mi) if (!add_mesh(mi)) return false;
        if (!add_instances()) return false;
        certify_convex_instances();
        if (!add_top_level()) return false;
        add_sweep_table();
        if (!add_environment()) return false;
        finish_header();
        return true;
    }

    // ---- 1. the checks that need nothing built (meshes and instances are checked where they are built)
    bool check_description() {
        if (d.material_count == 0 || !d.materials) return fail("scene needs at least the error material (index 0)");
        if (d.camera_count == 0 || !d.cameras) return fail("scene has no camera");
        if (d.environment.kind != PT_ENV_CONSTANT && d.environment.kind != PT_ENV_SUN && d.environment.kind != PT_ENV_HDR) return fail("unknown environment kind");
        if (d.environment.kind == PT_ENV_HDR) {
            if (d.environment.texstack < 0 || (uint32_t)d.environment.texstack >= d.texstack_count) return fail("environment texstack out of range");
            if (d.environment.importance_width < 0 || d.environment.importance_height < 0 || d.environment.importance_width > 16384 || d.environment.importance_height > 16384) return fail("bad importance map size");
            if (d.environment.importance_luminance_curve >= (int32_t)d.curve_count) return fail("importance luminance curve out of range");
        } else if (d.environment.curve < 0 || (uint32_t)d.environment.curve >= d.curve_count) return fail("environment curve index out of range");
        if (const char* bad = check_curves(d.curves, d.curve_count, d.curve_data_count)) return fail(bad);
        for (uint32_t i = 0; i < d.material_count; ++i) {
            const pt_material& m = d.materials[i];
            switch (m.kind) {
                case PT_MATERIAL_LAMBERTIAN: if (m.texstack < 0 || (uint32_t)m.texstack >= d.texstack_count) return fail("lambertian texstack out of range"); break;
                case PT_MATERIAL_GGX: if (!curve_ok(m.curve_eta) || !curve_ok(m.curve_eta_o) || !curve_ok(m.curve_kappa)) return fail("ggx curve out of range");
                    if (!(m.alpha > 0.0f)) return fail("ggx alpha must be positive"); break;
                case PT_MATERIAL_DIFFUSE_LIGHT: case PT_MATERIAL_SHARP_LIGHT: if (!curve_ok(m.curve_emit) || !curve_ok(m.curve_bounce)) return fail("light curve out of range"); break;
                case PT_MATERIAL_PASSTHROUGH: if (!curve_ok(m.curve_bounce)) return fail("passthrough colour curve out of range"); break;
                default: return fail("unknown material kind");
            }
            if (m.outer_medium < 0 || m.inner_medium < 0 || (uint32_t)m.outer_medium > d.medium_count || (uint32_t)m.inner_medium > d.medium_count) return fail("material medium id out of range");
        }
        if (d.medium_count > 255) return fail("more than 255 mediums");   // MediumId is a u8 (src/prelude.rs)
        if (d.medium_count && !d.mediums) return fail("mediums missing");
        for (uint32_t i = 0; i < d.medium_count; ++i) {
            const pt_medium& m = d.mediums[i];
            if (m.kind == PT_MEDIUM_HG) { if (!curve_ok(m.curve_g) || !curve_ok(m.curve_sigma_a) || !curve_ok(m.curve_sigma_s)) return fail("HG medium curve out of range"); }
            else if (m.kind == PT_MEDIUM_RAYLEIGH) { if (!curve_ok(m.curve_ior)) return fail("Rayleigh medium curve out of range"); }
            else return fail("unknown medium kind");
        }
        for (uint32_t i = 0; i < d.texstack_count; ++i) {
            const pt_texstack& t = d.texstacks[i];
            if (t.first_layer < 0 || t.layer_count < 0 || (uint32_t)(t.first_layer + t.layer_count) > d.layer_count) return fail("texstack layers out of range");
            for (int l = 0; l < t.layer_count; ++l) {
                const pt_texture_layer& L = d.layers[t.first_layer + l];
                if (L.kind != PT_TEXTURE1 && L.kind != PT_TEXTURE4) return fail("unknown texture layer kind");
                if (L.width <= 0 || L.height <= 0) return fail("empty texture");
                size_t n = (size_t)L.width * L.height * (L.kind == PT_TEXTURE4 ? 4 : 1);
                if (L.data_offset + n > d.texture_data_count) return fail("texture data out of range");
                for (int k = 0; k < (L.kind == PT_TEXTURE4 ? 4 : 1); ++k) if (!curve_ok(L.curves[k])) return fail("texture curve out of range");
                if (L.data_offset + n > 0xffffffffull) return fail("texture data too large");
            }
        }
        return true;
    }

    // the empty header, the texels, the cameras and the curves
    void begin(bool curve_tables, uint32_t* curve_table_words) {
        w.assign(PT_HDR_WORDS, 0);
        hs->tex.assign(d.texture_data, d.texture_data + d.texture_data_count);
        if (hs->tex.empty()) hs->tex.push_back(0.0f);
        hs->cameras.assign(d.cameras, d.cameras + d.camera_count);
        flatten_curves(d.curves, d.curve_count, d.curve_data, curve_tables, w, &curve_off, curve_table_words);
        w[PT_HDR_CURVE_OFF] = d.curve_count ? curve_off[0] : 0; w[PT_HDR_CURVE_COUNT] = d.curve_count;
        hs->curve_offsets = curve_off;
    }

    // ---- 2. texstacks
    void add_texstacks() {
        pad16(w);
        ts_off.assign(d.texstack_count, 0);
        for (uint32_t i = 0; i < d.texstack_count; ++i) {
            const pt_texstack& t = d.texstacks[i];
            ts_off[i] = (uint32_t)w.size();
            w.push_back((uint32_t)t.layer_count);
            for (int l = 0; l < t.layer_count; ++l) {
                const pt_texture_layer& L = d.layers[t.first_layer + l];
                w.push_back((uint32_t)L.kind);
                for (int k = 0; k < 4; ++k) w.push_back((L.kind == PT_TEXTURE4 || k == 0) ? curve_off[L.curves[k]] : 0);
                w.push_back((uint32_t)L.width); w.push_back((uint32_t)L.height); w.push_back((uint32_t)L.data_offset);
            }
        }
    }

    // ---- 3. materials
    void add_materials() {
        pad16(w);
        w[PT_HDR_MATERIAL_OFF] = (uint32_t)w.size(); w[PT_HDR_MATERIAL_COUNT] = d.material_count;
        for (uint32_t i = 0; i < d.material_count; ++i) {
            const pt_material& m = d.materials[i];
            uint32_t r[PT_MAT_WORDS] = {0};
            r[PT_MAT_KIND] = (uint32_t)m.kind;
            r[PT_MAT_ALPHA] = fbits(m.alpha);
            r[PT_MAT_SHARPNESS] = fbits(1.0f + std::fabs(m.sharpness));  // SharpLight::new, sharp_light.rs:26
            r[PT_MAT_SIDEDNESS] = (uint32_t)m.sidedness;
            if (m.kind == PT_MATERIAL_LAMBERTIAN) r[PT_MAT_TEXSTACK] = ts_off[m.texstack];
            if (m.kind == PT_MATERIAL_GGX) {
                r[PT_MAT_ETA] = curve_off[m.curve_eta]; r[PT_MAT_ETA_O] = curve_off[m.curve_eta_o]; r[PT_MAT_KAPPA] = curve_off[m.curve_kappa];
                // GGX::new: metallic = kappa.evaluate_integral(BOUNDED_VISIBLE_RANGE, 100, false) > 0 (ggx.rs:205)
                ptd::SceneView view{w.data(), hs->tex.data()};
                const float sum = visible_range_sum([&](int k) { return ptd::curve_eval(view, curve_off[m.curve_kappa], visible_lambda(k)); });
                r[PT_MAT_METALLIC] = sum > 0.0f ? 1u : 0u;
            }
            if (m.kind == PT_MATERIAL_DIFFUSE_LIGHT || m.kind == PT_MATERIAL_SHARP_LIGHT) { r[PT_MAT_EMIT] = curve_off[m.curve_emit]; r[PT_MAT_BOUNCE] = curve_off[m.curve_bounce]; }
            if (m.kind == PT_MATERIAL_PASSTHROUGH) r[PT_MAT_BOUNCE] = curve_off[m.curve_bounce];
            r[PT_MAT_MEDIUMS] = (uint32_t)m.outer_medium | (uint32_t)m.inner_medium << 8;
            w.insert(w.end(), r, r + PT_MAT_WORDS);
        }
    }

    // ---- 4. mediums (World::mediums): read by the medium-aware walk only
    void add_mediums() {
        if (!d.medium_count) return;
        pad16(w);
        w[PT_HDR_MEDIUM_OFF] = (uint32_t)w.size(); w[PT_HDR_MEDIUM_COUNT] = d.medium_count;
        for (uint32_t i = 0; i < d.medium_count; ++i) {
            const pt_medium& m = d.mediums[i];
            uint32_t r[PT_MEDIUM_WORDS] = {0};
            r[PT_MED_KIND] = (uint32_t)m.kind;
            if (m.kind == PT_MEDIUM_HG) { r[PT_MED_G] = curve_off[m.curve_g]; r[PT_MED_SIGMA_A] = curve_off[m.curve_sigma_a]; r[PT_MED_SIGMA_S] = curve_off[m.curve_sigma_s]; }
            else r[PT_MED_IOR] = curve_off[m.curve_ior];
            r[PT_MED_CORRECTIVE] = fbits(m.corrective_factor);
            w.insert(w.end(), r, r + PT_MEDIUM_WORDS);
        }
    }

    // ---- 5. one mesh: its BVH over triangles (Mesh::init, mesh.rs:283-305) and the gathered triangle records into the mesh section, its record into the core
    bool add_mesh(uint32_t mi) {
        const pt_mesh& m = d.meshes[mi];
        if ((size_t)m.vertex_offset + m.vertex_count > d.vertex_count) return fail("mesh vertices out of range");
        if ((size_t)m.index_offset + 3 * (size_t)m.face_count > d.index_count) return fail("mesh indices out of range");
        if (m.normal_offset >= 0 && (size_t)m.normal_offset + m.vertex_count > d.normal_count) return fail("mesh normals out of range");
        if (m.face_material_offset >= 0 && (size_t)m.face_material_offset + m.face_count > d.face_material_count) return fail("mesh face materials out of range");
        if (m.face_count == 0) return fail("mesh without faces");
        MeshWork k{m, d.vertices + 3 * (size_t)m.vertex_offset, d.indices + m.index_offset, meshes[mi]};
        if (!mesh_bvh(mi, k) || !mesh_triangles(k)) return false;
        if (m.normal_offset < 0) mesh_face_normals(k); else mesh_vertex_normals(k);
        mesh_emissive_areas(k);
        mesh_permuted_copies(k);
        mesh_leaf_list(k);
        mesh_group_boxes(k);
        uint32_t rec[PT_MESH_WORDS] = {k.out.node_off, k.out.node_count, k.out.tri_off, k.normal_off, m.face_count, k.leaf_off, k.leaf_count, k.group_off};
        for (int q = 8; q < PT_MESH_WORDS; ++q) rec[q] = 0u;
        mesh_inner_ball(mi, k, rec);
        mesh_slabs(k, rec);
        k.out.record = (uint32_t)w.size();
        w.insert(w.end(), rec, rec + PT_MESH_WORDS);
        return true;
    }

    bool mesh_bvh(uint32_t mi, MeshWork& k) {
        Box mb = box_empty();
        for (uint32_t v = 0; v < k.m.vertex_count; ++v) box_grow(mb, k.V + 3 * v);  // Mesh::new bounding box over all vertices
        k.out.box = mb;
        std::vector<Box> tb(k.m.face_count);
        for (uint32_t f = 0; f < k.m.face_count; ++f) {
            const uint32_t* ix = k.ix + 3 * (size_t)f;
            for (int c = 0; c < 3; ++c) if (ix[c] >= k.m.vertex_count) return fail("mesh index out of range");
            Box b = box_of_corners(k.V + 3 * ix[0], k.V + 3 * ix[1]); box_grow(b, k.V + 3 * ix[2]);  // mesh.rs:57-64
            tb[f] = b;
        }
        pad16(md);
        k.out.node_off = (uint32_t)md.size();
        // (a node's exit link is 27 bits of a word that also holds the form of its box test, pt_blob.h: 2 n - 1 nodes must fit)
        if (2ull * tb.size() >= (1ull << 27)) { *err = "mesh " + std::to_string(mi) + ": " + std::to_string(tb.size()) + " triangles make a BVH of 2^27 or more nodes (the skip-link field is 27 bits)"; return false; }
        BvhBuilder bb(tb, k.nodes); bb.build();
        md.insert(md.end(), k.nodes.begin(), k.nodes.end());
        k.out.node_count = (uint32_t)(k.nodes.size() / PT_NODE_WORDS);
        return true;
    }

    bool mesh_triangles(MeshWork& k) {
        k.out.tri_off = (uint32_t)md.size();
        for (uint32_t f = 0; f < k.m.face_count; ++f) {
            const uint32_t* ix = k.ix + 3 * (size_t)f;
            uint32_t mat = k.m.face_material_offset >= 0 ? d.face_materials[k.m.face_material_offset + f] : PT_MATERIAL_ID(PT_TAG_MATERIAL, 0);
            if (!material_ok(mat) || mat == PT_MATERIAL_NONE) return fail("mesh face material out of range");
            if (PT_MATERIAL_TAG(mat) == PT_TAG_LIGHT) k.out.light_faces.push_back(f);
            for (int c = 0; c < 3; ++c) {
                const float* p = k.V + 3 * ix[c];
                md.push_back(fbits(p[0])); md.push_back(fbits(p[1])); md.push_back(fbits(p[2])); md.push_back(c == 0 ? mat : 0u);
            }
        }
        return true;
    }

    // Without vertex normals a hit's normal is the face's: normalize(cross(p0 - p2, p1 - p2)) (mesh.rs:176-181), normalised once more by
    // HitRecord::new (hittable.rs:30-39).  Both depend on the triangle alone, so they are computed here, with the very operations
    // hit_record would use (same header, no contraction, IEEE division and square root on both sides), and the second vertex's spare
    // word points at the result: two square roots, six divisions and a cross product less per closest hit.
    void mesh_face_normals(MeshWork& k) {
        pad16(md);
        const uint32_t fn_off = (uint32_t)md.size();
        for (uint32_t f = 0; f < k.m.face_count; ++f) {
            const size_t at = k.out.tri_off + (size_t)f * PT_TRI_WORDS;
            auto vert = [&](int c) { return ptd::f3(pt_u2f(md[at + 4 * c]), pt_u2f(md[at + 4 * c + 1]), pt_u2f(md[at + 4 * c + 2])); };
            const ptd::F3 p0 = vert(0), p1 = vert(1), p2 = vert(2);
            const ptd::F3 n = ptd::normalize(ptd::normalize(ptd::cross(ptd::sub(p0, p2), ptd::sub(p1, p2))));
            md[at + 7] = fn_off + 4 * f;   // (the second vertex' spare word)
            md.push_back(fbits(n.x)); md.push_back(fbits(n.y)); md.push_back(fbits(n.z)); md.push_back(0u);
        }
    }

    void mesh_vertex_normals(MeshWork& k) {
        const float* N = d.normals + 3 * (size_t)k.m.normal_offset;
        k.normal_off = (uint32_t)md.size();
        for (uint32_t f = 0; f < k.m.face_count; ++f) {
            const uint32_t* ix = k.ix + 3 * (size_t)f;
            for (int c = 0; c < 3; ++c) { const float* p = N + 3 * ix[c]; md.push_back(fbits(p[0])); md.push_back(fbits(p[1])); md.push_back(fbits(p[2])); md.push_back(0u); }
        }
    }

    // A_f of every emissive face into the spare word of its normal record (pt_blob.h PT_HDR_LIGHT_FACE_OFF): the face normal's, or the first vertex normal's
    void mesh_emissive_areas(MeshWork& k) {
        for (uint32_t f : k.out.light_faces) {
            const size_t at = k.out.tri_off + (size_t)f * PT_TRI_WORDS;
            const uint32_t spare = k.normal_off != 0u ? k.normal_off + f * PT_TRI_WORDS + 3u : md[at + 7] + 3u;
            md[spare] = fbits(triangle_area(k.V, k.ix + 3 * (size_t)f));
        }
    }

    // permuted copies of the triangles of a mesh small enough to be taken into the sweep table (pt_blob.h)
    void mesh_permuted_copies(MeshWork& k) {
        if (!(k.m.face_count < PT_SWEEP_MAX_BITS)) return;
        for (int variant = 0; variant < 2; ++variant) {
            (variant == 0 ? k.out.perm0 : k.out.perm1) = (uint32_t)md.size() - k.out.tri_off;
            for (uint32_t f = 0; f < k.m.face_count; ++f)
                for (int c = 0; c < 3; ++c) {
                    const size_t at = k.out.tri_off + f * PT_TRI_WORDS + 4 * c;
                    const uint32_t q[4] = {md[at], md[at + 1], md[at + 2], md[at + 3]};  // (copied: push_back reallocates)
                    if (variant == 0) { md.push_back(q[1]); md.push_back(q[2]); md.push_back(q[0]); }   // (y, z, x)
                    else { md.push_back(q[2]); md.push_back(q[0]); md.push_back(q[1]); }               // (z, x, y)
                    md.push_back(q[3]);
                }
        }
    }

    // leaf list for mesh_sweep: the leaf boxes alone, in pre-order (a dense wave of rays inside a mesh of a few hundred
    // triangles tests them all, 64 at a time, instead of walking the tree lane by lane)
    void mesh_leaf_list(MeshWork& k) {
        if (!(k.m.face_count <= PT_MESH_SWEEP_MAX)) return;
        pad16(md);
        k.leaf_off = (uint32_t)md.size();
        for (size_t n = 0; n < k.nodes.size() / PT_NODE_WORDS; ++n) {
            const uint32_t* nd = &k.nodes[n * PT_NODE_WORDS];
            if (nd[7] == PT_NODE_INNER) continue;
            uint32_t rec[8] = {nd[0], nd[1], nd[2], k.out.tri_off + nd[7] * PT_TRI_WORDS, nd[4], nd[5], nd[6], PT_NODE_CODE(nd[3])};   // [7]: the form of the box test
            md.insert(md.end(), rec, rec + 8);
            ++k.leaf_count;
        }
    }

    // group boxes for mesh_sweep: a ray tests the group boxes first and then only the leaves of the groups it enters (a box that
    // holds a leaf's box passes AABB::hit whenever the leaf's does, like a BVH ancestor)
    void mesh_group_boxes(MeshWork& k) {
        if (!(k.leaf_count > PT_MESH_GROUP_MIN)) return;
        pad16(md);
        k.group_off = (uint32_t)md.size();
        for (uint32_t first = 0; first < k.leaf_count; first += PT_MESH_GROUP) {
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (uint32_t t = first; t < k.leaf_count && t < first + PT_MESH_GROUP; ++t) {
                const uint32_t* lf = &md[k.leaf_off + t * 8u];
                for (int c = 0; c < 3; ++c) { mn[c] = std::fmin(mn[c], bits_f(lf[c])); mx[c] = std::fmax(mx[c], bits_f(lf[4 + c])); }
            }
            const uint32_t flat = box_test_form(mn, mx) != 0u ? 1u : 0u;
            uint32_t rec[8] = {fbits(mn[0]), fbits(mn[1]), fbits(mn[2]), 0u, fbits(mx[0]), fbits(mx[1]), fbits(mx[2]), flat};
            md.insert(md.end(), rec, rec + 8);
        }
    }

    // the inner sphere of a closed mesh without light faces (pt_blob.h PT_MESH_INNER_*), and the mesh's reach
    void mesh_inner_ball(uint32_t mi, MeshWork& k, uint32_t* rec) {
        const pt_mesh& m = k.m;
        const Box& mb = k.out.box;
        float c[3] = {0.0f, 0.0f, 0.0f}, r = 0.0f;
        std::vector<float> more;
        if (k.out.light_faces.empty() && m.face_count >= 4 && m.face_count <= 200000 && inner_sphere(k.V, m.vertex_count, k.ix, m.face_count, mb, c, &r, &more)) {
            rec[PT_MESH_INNER_C] = fbits(c[0]); rec[PT_MESH_INNER_C + 1] = fbits(c[1]); rec[PT_MESH_INNER_C + 2] = fbits(c[2]); rec[PT_MESH_INNER_R] = fbits(r);
            if (!more.empty()) {   // (in the core section, in front of the record: four words a ball)
                pad16(w);
                rec[PT_MESH_MORE_OFF] = (uint32_t)w.size(); rec[PT_MESH_MORE_COUNT] = (uint32_t)(more.size() / 4);
                for (float x : more) w.push_back(fbits(x));
            }
        }
        if (verbose) fprintf(stderr, "mesh %u: %u faces, inner ball centre (%g, %g, %g) radius %g (0 = none)\n", mi, m.face_count, c[0], c[1], c[2], r);
        const double dx = (double)mb.mx[0] - mb.mn[0], dy = (double)mb.mx[1] - mb.mn[1], dz = (double)mb.mx[2] - mb.mn[2];
        rec[PT_MESH_REACH] = fbits((float)(std::sqrt(dx * dx + dy * dy + dz * dz) * 1.0001));
    }

    // the slabs of the 26-DOP beyond the box (pt_blob.h PT_MESH_DOP_*), in the core section in front of the record: every vertex, f64, widened by 1e-3 of the
    // slab's width and rounded outward
    void mesh_slabs(MeshWork& k, uint32_t* rec) {
        static const int dirs[PT_MESH_DOP_DIRS][3] = {{1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1}, {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
        pad16(w);
        const uint32_t dop_off = (uint32_t)w.size();
        bool centred = true;   // (no slab lies more than 500 of its own widths from the mesh's origin: mesh_surely_missed's error budget)
        for (int s = 0; s < PT_MESH_DOP_DIRS; ++s) {
            double lo = INFINITY, hi = -INFINITY;
            for (uint32_t v = 0; v < k.m.vertex_count; ++v) {
                const double x = (double)dirs[s][0] * k.V[3 * v] + (double)dirs[s][1] * k.V[3 * v + 1] + (double)dirs[s][2] * k.V[3 * v + 2];
                lo = std::fmin(lo, x); hi = std::fmax(hi, x);
            }
            const double margin = 1e-3 * (hi - lo);
            const float flo = std::nextafterf((float)(lo - margin), -INFINITY), fhi = std::nextafterf((float)(hi + margin), INFINITY);
            w.push_back(fbits(flo)); w.push_back(fbits(fhi));
            centred = centred && std::isfinite(lo) && std::isfinite(hi) && hi > lo && std::fmax(std::fabs(lo), std::fabs(hi)) <= 500.0 * (hi - lo);
        }
        w.push_back(0u);
        rec[PT_MESH_DOP_OFF] = centred ? dop_off : 0u;
        pad16(w);
    }

    // ---- 6. instances + their world boxes (Instance::aabb, instance.rs:65-72; Matrix4x4 * AABB, aabb.rs:116-138), and the light list
    bool add_instances() {
        pad16(w);
        w[PT_HDR_INSTANCE_OFF] = (uint32_t)w.size(); w[PT_HDR_INSTANCE_COUNT] = d.instance_count;
        ibox.resize(d.instance_count);
        for (uint32_t i = 0; i < d.instance_count; ++i) {
            const pt_instance& in = d.instances[i];
            if (!material_ok(in.material)) return fail("instance material out of range");
            uint32_t r[PT_INST_WORDS] = {0};
            r[PT_INST_KIND] = (uint32_t)in.kind;
            r[PT_INST_FLAGS] = (in.has_transform ? 1u : 0u) | (in.two_sided ? 2u : 0u) | (((uint32_t)in.axis & 3u) << 2);
            r[PT_INST_MATERIAL] = in.material;
            for (int k = 0; k < 3; ++k) r[PT_INST_ORIGIN + k] = fbits(in.origin[k]);
            r[PT_INST_RADIUS] = fbits(in.radius);
            r[PT_INST_SIZE] = fbits(in.size[0]); r[PT_INST_SIZE + 1] = fbits(in.size[1]);
            for (int k = 0; k < 12; ++k) { r[PT_INST_FORWARD + k] = fbits(in.forward[k]); r[PT_INST_REVERSE + k] = fbits(in.reverse[k]); }
            switch (in.kind) {
                case PT_SHAPE_RECT: if (!(in.size[0] > 0.0f && in.size[1] > 0.0f) || in.axis < 0 || in.axis > 2) return fail("bad rect"); break;
                case PT_SHAPE_SPHERE: if (!(in.radius > 0.0f)) return fail("bad sphere"); break;
                case PT_SHAPE_DISK: if (!(in.radius > 0.0f)) return fail("bad disk"); break;
                case PT_SHAPE_MESH:
                    if (in.mesh < 0 || (uint32_t)in.mesh >= d.mesh_count) return fail("instance mesh out of range");
                    r[PT_INST_MESH] = meshes[in.mesh].record; break;
                default: return fail("unknown shape kind");
            }
            Box b = in.kind == PT_SHAPE_MESH ? meshes[in.mesh].box : shape_box(in, in.radius / 2.0f);   // (a disk's: radius / 2, the reference's quirk kept)
            if (in.has_transform) b = transformed_box(b, in.forward);
            ibox[i] = b;
            w.insert(w.end(), r, r + PT_INST_WORDS);
            // World::new light list (world/mod.rs:42-66)
            // (an emissive face is a light of its own: the j-th entry of the instance's run is the mesh's j-th emissive face)
            if (in.kind == PT_SHAPE_MESH) {
                for (uint32_t f : meshes[in.mesh].light_faces) { lights.push_back(i); light_faces.push_back(meshes[in.mesh].tri_off + f * PT_TRI_WORDS); }
            } else {
                uint32_t mid = in.material == PT_MATERIAL_NONE ? PT_MATERIAL_ID(PT_TAG_MATERIAL, 0) : in.material;
                if (PT_MATERIAL_TAG(mid) == PT_TAG_LIGHT) { lights.push_back(i); light_faces.push_back(0u); }
            }
        }
        return true;
    }

    // ---- 7. convex closed mesh instances (pt_blob.h PT_INST_CONVEX_*): certified once per instance, in world space; their faces' flags into the triangle records
    bool lightish(uint32_t i) const {   // can a hit on instance i carry a Light tag
        const pt_instance& in = d.instances[i];
        if (in.material != PT_MATERIAL_NONE) return PT_MATERIAL_TAG(in.material) == PT_TAG_LIGHT;
        return in.kind == PT_SHAPE_MESH && !meshes[in.mesh].light_faces.empty();
    }
    // (a Disk's box in the tree is the reference's, half the radius — disk.rs:24-28, a kept quirk — and does not hold the disk: the certificate's "no light near the body"
    // is about where the light IS.  Found by the soak, seed 197995: a lit disk whose reference box cleared a glass cube's while its rim reached into the cube.)
    Box true_box(uint32_t i) const {
        const pt_instance& in = d.instances[i];
        if (in.kind != PT_SHAPE_DISK) return ibox[i];
        const Box b = shape_box(in, in.radius);
        return in.has_transform ? transformed_box(b, in.forward) : b;
    }
    // The faces' flag words ride in the MESH's triangle records: with several certified instances of one mesh a face keeps the weaker of their claims (the larger
    // outward threshold — 0, "none", being the largest —, the weaker inward flag: whole face > inside only > none).
    static void merge_face_flags(std::vector<uint32_t>& mf, const std::vector<uint32_t>& face_flags) {
        if (mf.empty()) { mf = face_flags; return; }
        for (size_t f = 0; f < mf.size(); ++f) {
            const uint32_t ta = mf[f] >> PT_TRI_OUT_SHIFT, tb = face_flags[f] >> PT_TRI_OUT_SHIFT, t = (ta == 0u || tb == 0u) ? 0u : (ta > tb ? ta : tb);
            const uint32_t ia = mf[f] & 3u, ib = face_flags[f] & 3u;
            const uint32_t in_bits = (ia == 0u || ib == 0u) ? 0u : ((ia == PT_TRI_IN_SAFE && ib == PT_TRI_IN_SAFE) ? PT_TRI_IN_SAFE : PT_TRI_IN_SAFE_INNER);
            mf[f] = t << PT_TRI_OUT_SHIFT | in_bits;
        }
    }
    void certify_convex_instances() {
        std::vector<Box> light_boxes;
        for (uint32_t i = 0; i < d.instance_count; ++i) if (lightish(i)) light_boxes.push_back(true_box(i));
        std::vector<int> mesh_closed(d.mesh_count, -1);
        double work_left = 4e8;   // (the certificate is O(faces x vertices + faces^2) per INSTANCE: a scene of thousands of mesh instances certifies the first of them — about a second — and leaves the rest alone)
        bool any = false;
        for (uint32_t i = 0; i < d.instance_count && d.instance_count <= 65536u; ++i) {   // (a hit's instance word and the mark a ray carries name the instance in 16 bits: a scene of more instances takes no certificate)
            const pt_instance& in = d.instances[i];
            if (in.kind != PT_SHAPE_MESH || lightish(i)) continue;
            const pt_mesh& m = d.meshes[in.mesh];
            const float* V = d.vertices + 3 * (size_t)m.vertex_offset;
            const uint32_t* ix = d.indices + m.index_offset;
            if (m.face_count > 4096) continue;
            if (mesh_closed[in.mesh] < 0) mesh_closed[in.mesh] = mesh_is_closed(V, m.vertex_count, ix, m.face_count, meshes[in.mesh].box) ? 1 : 0;
            if (!mesh_closed[in.mesh]) continue;
            const double work = (double)m.face_count * m.vertex_count + 4.0 * (double)m.face_count * m.face_count;
            if (work > work_left) continue;
            work_left -= work;
            std::vector<uint32_t> face_flags;
            uint32_t cf = convex_certificate(V, m.vertex_count, ix, m.face_count, m.normal_offset >= 0 ? d.normals + 3 * (size_t)m.normal_offset : nullptr, in, ibox[i], light_boxes, &face_flags);
            if (cf != 0u) merge_face_flags(meshes[in.mesh].face_flags, face_flags);
            if (verbose) fprintf(stderr, "instance %u: mesh %d, convex certificate %s%s\n", i, in.mesh, (cf & PT_INST_CONVEX_OUT) ? "OUT " : "none", (cf & PT_INST_CONVEX_IN) ? "IN" : "");
            w[w[PT_HDR_INSTANCE_OFF] + i * PT_INST_WORDS + PT_INST_FLAGS] |= cf;
            any = any || cf != 0u;
        }
        if (any) w[PT_HDR_FLAGS] |= PT_FLAG_CONVEX;
        {   // PT_HDR_CONVEX_INST: the only OUT-certified instance, if there is exactly one
            uint32_t count = 0, which = 0;
            for (uint32_t i = 0; i < d.instance_count; ++i) if (w[w[PT_HDR_INSTANCE_OFF] + i * PT_INST_WORDS + PT_INST_FLAGS] & PT_INST_CONVEX_OUT) { ++count; which = i; }
            w[PT_HDR_CONVEX_INST] = count == 1 ? which + 1u : 0u;
        }
        for (const MeshBuilt& mesh : meshes) {   // the faces' flag words (PT_TRI_FLAGS) into the triangle records, and into their permuted copies
            for (size_t f = 0; f < mesh.face_flags.size(); ++f) {
                const uint32_t word = mesh.face_flags[f];
                md[mesh.tri_off + f * PT_TRI_WORDS + PT_TRI_FLAGS] = word;
                if (mesh.perm0 != 0u) { md[mesh.tri_off + mesh.perm0 + f * PT_TRI_WORDS + PT_TRI_FLAGS] = word; md[mesh.tri_off + mesh.perm1 + f * PT_TRI_WORDS + PT_TRI_FLAGS] = word; }
            }
        }
    }

    // ---- 8. the top-level BVH over instances, the sphere nodes' culling margins and the three light lists
    bool add_top_level() {
        pad16(w);
        if (2ull * d.instance_count >= (1ull << 27)) { *err = std::to_string(d.instance_count) + " instances make a top-level BVH of 2^27 or more nodes (the skip-link field is 27 bits)"; return false; }
        BvhBuilder bb(ibox, top_nodes);
        bb.no_cull.assign(d.instance_count, 0);
        for (uint32_t i = 0; i < d.instance_count; ++i) bb.no_cull[i] = d.instances[i].kind == PT_SHAPE_SPHERE;
        bb.sphere_radius.assign(d.instance_count, 0.0f);
        for (uint32_t i = 0; i < d.instance_count; ++i)
            if (d.instances[i].kind == PT_SHAPE_SPHERE) bb.sphere_radius[i] = d.instances[i].has_transform ? INFINITY : d.instances[i].radius;
        bb.build();
        w[PT_HDR_TOP_NODE_OFF] = (uint32_t)w.size(); w[PT_HDR_TOP_NODE_COUNT] = (uint32_t)(top_nodes.size() / PT_NODE_WORDS);
        uint32_t top = (uint32_t)w.size();
        w.insert(w.end(), top_nodes.begin(), top_nodes.end());
        pad16(w);
        {   // PT_HDR_TOP_MARGIN: the sphere nodes' culling margins, one float per top-level node
            bool any = false;
            for (float m : bb.node_margin) any = any || m != 0.0f;
            if (any) {
                bb.node_margin.resize(top_nodes.size() / PT_NODE_WORDS, 0.0f);
                w[PT_HDR_TOP_MARGIN] = (uint32_t)w.size();
                for (float m : bb.node_margin) w.push_back(fbits(m));
                pad16(w);
            }
        }
        w[PT_HDR_LIGHT_OFF] = (uint32_t)w.size(); w[PT_HDR_LIGHT_COUNT] = (uint32_t)lights.size();
        w.insert(w.end(), lights.begin(), lights.end());
        pad16(w);
        w[PT_HDR_LIGHT_NODE_OFF] = (uint32_t)w.size();
        for (uint32_t l : lights) w.push_back(top + bb.leaf_of_shape[l] * PT_NODE_WORDS);
        bool face_lights = false;
        for (uint32_t t : light_faces) face_lights = face_lights || t != 0u;
        if (face_lights) {   // (only a scene with emissive mesh faces has the list: every other scene's blob is word for word what it was before them)
            pad16(w);
            w[PT_HDR_LIGHT_FACE_OFF] = (uint32_t)w.size();
            w.insert(w.end(), light_faces.begin(), light_faces.end());
        }
        return true;
    }

    // ---- 9. leaf sweep table (world_hit_sweep): the leaf boxes of both levels in traversal pre-order, as far as 64 mask bits
    // go.  Every instance takes a bit; the triangle leaves of mesh instances are taken in ("inlined") smallest mesh first
    // while they fit; the remaining mesh instances keep only their own bit and their BVH is walked when that bit is hit.
    std::vector<char> walked_instances() const {
        std::vector<char> walked(d.instance_count, 0);
        size_t sweep_bits = d.instance_count;
        std::vector<uint32_t> mesh_instances;
        for (uint32_t i = 0; i < d.instance_count; ++i) if (d.instances[i].kind == PT_SHAPE_MESH) mesh_instances.push_back(i);
        std::stable_sort(mesh_instances.begin(), mesh_instances.end(), [&](uint32_t a, uint32_t b) {
            return d.meshes[d.instances[a].mesh].face_count < d.meshes[d.instances[b].mesh].face_count; });
        for (uint32_t i : mesh_instances) {
            size_t faces = d.meshes[d.instances[i].mesh].face_count;
            if (sweep_bits + faces <= PT_SWEEP_MAX_BITS) sweep_bits += faces; else walked[i] = 1;
        }
        return walked;
    }

    void add_sweep_table() {
        if (!(d.instance_count > 0 && d.instance_count <= PT_SWEEP_MAX_BITS)) return;
        const std::vector<char> walked = walked_instances();
        pad16(w);
        std::vector<uint32_t> order;  // top-level leaf nodes in pre-order
        for (size_t k = 0; k < top_nodes.size() / PT_NODE_WORDS; ++k) if (top_nodes[k * PT_NODE_WORDS + 7] != PT_NODE_INNER) order.push_back((uint32_t)k);
        SweepTable t;
        t.off = (uint32_t)w.size();
        w.resize(w.size() + order.size() * PT_SWEEP_INST_WORDS, 0);
        for (size_t j = 0; j < order.size(); ++j) {
            const uint32_t* nd = &top_nodes[order[j] * PT_NODE_WORDS];
            sweep_instance(t, t.off + (uint32_t)j * PT_SWEEP_INST_WORDS, nd, walked[nd[7]] != 0);
        }
        // The instance records too may stand in any order (their masks carry the leaf order).  Those whose box test is all there is to do — no
        // triangle leaf with a test of its own: analytic shapes, the walls whose two triangles ride in the instance's mask, walked meshes — come
        // first, grouped by the form of the test: the sweep runs them through tight loops (pt_device.h sweep_masks), the others through the
        // general one.  A sphere is never culled (pt_device.h beyond) and stays with the general loop.
        std::vector<uint32_t> simple_code(order.size());   // 0..4: simple with that test form; 5: general
        for (size_t j = 0; j < order.size(); ++j) {
            const uint32_t kf = w[t.off + j * PT_SWEEP_INST_WORDS + 1];
            simple_code[j] = ((kf >> 24) == 0u && (kf & 0xffu) != PT_SHAPE_SPHERE) ? ((kf >> 11) & 7u) : 5u;
        }
        const std::array<uint32_t, 6> counts = regroup_records(w, t.off, PT_SWEEP_INST_WORDS, simple_code, t.bits);
        w[PT_HDR_SWEEP_SIMPLE] = counts[0] | counts[1] << 8 | counts[2] << 16 | counts[3] << 24;   // (at most 64 instances)
        w[PT_HDR_SWEEP_SIMPLE + 1] = counts[4];
        for (size_t k = 0; k < t.root_of.size(); ++k)
            if (t.root_of[k] != (int)k) {
                uint64_t m = 1ull << k;
                t.bits[(size_t)t.root_of[k] * PT_SWEEP_BIT_WORDS + 4] |= (uint32_t)m; t.bits[(size_t)t.root_of[k] * PT_SWEEP_BIT_WORDS + 5] |= (uint32_t)(m >> 32);
            }
        pad16(w);
        w[PT_HDR_SWEEP_BITS_OFF] = (uint32_t)w.size();
        w.insert(w.end(), t.bits.begin(), t.bits.end());
        w[PT_HDR_SWEEP_MESH_MASK] = (uint32_t)t.mesh_mask; w[PT_HDR_SWEEP_MESH_MASK + 1] = (uint32_t)(t.mesh_mask >> 32);
        w[PT_HDR_SWEEP_OWNER_MASK] = (uint32_t)t.owner_mask; w[PT_HDR_SWEEP_OWNER_MASK + 1] = (uint32_t)(t.owner_mask >> 32);
        w[PT_HDR_SWEEP_OFF] = t.off; w[PT_HDR_SWEEP_COUNT] = (uint32_t)order.size();
        if (t.any_walked) w[PT_HDR_FLAGS] |= PT_FLAG_SWEEP_WALKS;
    }

    // One instance of the table: its own bit, the bits of its inlined triangle leaves, its record at word `e`.  nd: its top-level leaf node.
    void sweep_instance(SweepTable& t, uint32_t e, const uint32_t* nd, bool walked) {
        const uint32_t inst = nd[7];
        const pt_instance& in = d.instances[inst];
        const uint32_t rec_off = w[PT_HDR_INSTANCE_OFF] + inst * PT_INST_WORDS;
        const uint32_t form = box_test_form(nd, nd + 4);
        const uint32_t kf = (uint32_t)in.kind | (form != 0u ? 1u << 8 : 0u) | (in.has_transform ? 1u << 9 : 0u) | (walked ? PT_SWEEP_WALKED : 0u) | form << 11;
        const uint32_t first_bit = t.bit++;
        uint32_t own[PT_SWEEP_BIT_WORDS] = {rec_off, 0u, e + 4, kf | inst << 16, 0u, 0u, 0u, 0u};
        t.bits.insert(t.bits.end(), own, own + PT_SWEEP_BIT_WORDS);
        t.root_of.push_back((int)first_bit);
        if (in.kind == PT_SHAPE_MESH && walked) t.any_walked = true;
        if (in.kind != PT_SHAPE_MESH) t.owner_mask |= 1ull << first_bit;
        uint32_t tri_list = 0, tri_count = 0;
        std::vector<uint32_t> leader_code;   // per triangle-leaf record that keeps its own box test, in the order they stand from tri_list on: the form of that test
        if (in.kind == PT_SHAPE_MESH && !walked) {
            t.mesh_mask |= 1ull << first_bit;
            pad16(w);
            tri_list = (uint32_t)w.size();
            tri_count = sweep_triangle_bits(t, e, nd, kf, first_bit, &leader_code);
        }
        // the mask a box test sets: its own bit and the bits of the later leaves of this instance whose box is the same
        auto mask_of = [&](uint32_t leader_bit) { uint64_t m = 0; for (uint32_t b2 = first_bit; b2 < t.bit; ++b2) if (t.root_of[b2] == (int)leader_bit) m |= 1ull << b2; return m; };
        uint32_t b2 = first_bit + 1;
        for (size_t k = 0; k < leader_code.size(); ++k) {
            while (t.root_of[b2] != (int)b2) ++b2;
            const uint64_t m = mask_of(b2++);
            const uint32_t off = tri_list + (uint32_t)k * PT_SWEEP_TRI_WORDS;
            w[off + 3] = (uint32_t)m; w[off + 7] = (uint32_t)(m >> 32);
        }
        // The order of the box tests is free (the masks carry the leaf order): the records are grouped by the form of the test, so
        // that the sweep runs one specialised loop per form; [12] holds the sizes of the groups 0..3, the rest is group 4.
        const std::array<uint32_t, 6> groups = regroup_records(w, tri_list, PT_SWEEP_TRI_WORDS, leader_code, t.bits);
        const uint32_t group_sizes = groups[0] | groups[1] << 8 | groups[2] << 16 | groups[3] << 24;
        const uint64_t own_mask = mask_of(first_bit);
        {   // the instance's bits, all of them, in its own record (PT_INST_SWEEP_MASK: what a ray that may skip the instance drops from its leaf mask)
            const uint64_t all = (t.bit >= 64u ? ~0ull : (1ull << t.bit) - 1ull) & ~((1ull << first_bit) - 1ull);
            w[rec_off + PT_INST_SWEEP_MASK] = (uint32_t)all; w[rec_off + PT_INST_SWEEP_MASK + 1] = (uint32_t)(all >> 32);
        }
        uint32_t* r = &w[e];
        r[0] = rec_off; r[1] = kf | first_bit << 16 | (uint32_t)leader_code.size() << 24; r[2] = (uint32_t)own_mask; r[3] = (uint32_t)(own_mask >> 32);
        r[4] = nd[0]; r[5] = nd[1]; r[6] = nd[2]; r[7] = tri_list; r[8] = nd[4]; r[9] = nd[5]; r[10] = nd[6]; r[11] = tri_count;
        r[12] = group_sizes; r[13] = 0u; r[14] = inst; r[15] = 0u;
    }

    // The bits of an inlined mesh instance's triangle leaves, in the pre-order of the mesh's BVH.  A leaf whose box another bit of the instance tests already
    // copies that test; the others ("leaders") append a record with their box to w.  Returns the number of leaves.
    uint32_t sweep_triangle_bits(SweepTable& t, uint32_t e, const uint32_t* nd, uint32_t kf, uint32_t first_bit, std::vector<uint32_t>* leader_code) {
        const uint32_t inst = nd[7];
        const pt_instance& in = d.instances[inst];
        const MeshBuilt& mesh = meshes[in.mesh];
        const uint32_t rec_off = w[PT_HDR_INSTANCE_OFF] + inst * PT_INST_WORDS;
        uint32_t tri_count = 0;
        std::vector<std::array<uint32_t, 6>> seen;  // boxes of this instance's bits, index = bit - first_bit
        seen.push_back({nd[0], nd[1], nd[2], nd[4], nd[5], nd[6]});
        for (uint32_t k = 0; k < mesh.node_count; ++k) {
            uint32_t mn[PT_NODE_WORDS];
            for (int q = 0; q < PT_NODE_WORDS; ++q) mn[q] = md[mesh.node_off + k * PT_NODE_WORDS + q];
            if (mn[7] == PT_NODE_INNER) continue;
            std::array<uint32_t, 6> box = {mn[0], mn[1], mn[2], mn[4], mn[5], mn[6]};
            // the instance's own box is tested against the world ray: only an untransformed instance may share it
            uint32_t alias = 0;
            for (size_t q = in.has_transform ? 1 : 0; q < seen.size() && !alias; ++q) if (seen[q] == box) alias = first_bit + (uint32_t)q + 1;
            seen.push_back(box);
            t.root_of.push_back(alias ? t.root_of[alias - 1] : (int)t.bit);
            const uint32_t form = box_test_form(mn, mn + 4);
            uint32_t triw = mesh.tri_off + mn[7] * PT_TRI_WORDS, flat = form != 0u ? 1u : 0u;
            uint32_t box_words = e + 4;  // a copy of the instance's own box: settled with it, never looked up
            if (!alias) {
                leader_code->push_back(form);
                uint32_t rec[PT_SWEEP_TRI_WORDS] = {mn[0], mn[1], mn[2], 0u, mn[4], mn[5], mn[6], 0u};  // [3], [7]: the mask (sweep_instance)
                box_words = (uint32_t)w.size();
                w.insert(w.end(), rec, rec + PT_SWEEP_TRI_WORDS);
            } else if (t.root_of.back() != (int)first_bit) box_words = t.bits[(size_t)t.root_of.back() * PT_SWEEP_BIT_WORDS + 2];
            uint32_t tb[PT_SWEEP_BIT_WORDS] = {rec_off, triw, box_words, (kf & ~0x100u) | flat << 8 | inst << 16, 0u, 0u, mesh.perm0, mesh.perm1};
            t.bits.insert(t.bits.end(), tb, tb + PT_SWEEP_BIT_WORDS);
            if (in.has_transform) t.owner_mask |= 1ull << t.bit;
            ++tri_count; ++t.bit;
        }
        return tri_count;
    }

    // ---- 10. environment (World::new, world/mod.rs:69-81)
    bool add_environment() {
        pad16(w);
        const pt_environment& e = d.environment;
        w[PT_HDR_ENV_KIND] = (uint32_t)e.kind;
        w[PT_HDR_ENV_STRENGTH] = fbits(e.strength);
        w[PT_HDR_ENV_CURVE] = e.kind == PT_ENV_HDR ? 0u : curve_off[e.curve];
        if (e.kind == PT_ENV_HDR) {
            w[PT_HDR_ENV_TEXSTACK] = ts_off[e.texstack];
            for (int k = 0; k < 12; ++k) { w[PT_HDR_ENV_FORWARD + k] = fbits(e.rotation_forward[k]); w[PT_HDR_ENV_REVERSE + k] = fbits(e.rotation_reverse[k]); }
            if (e.importance_width > 0 && e.importance_height > 0 && e.strength > 0.0f && !bake_importance_map()) return false;
        }
        w[PT_HDR_ENV_ANGULAR] = fbits(e.angular_diameter);
        for (int k = 0; k < 3; ++k) w[PT_HDR_ENV_SUN_DIR + k] = fbits(e.sun_direction[k]);
        return true;
    }

    // ImportanceMap::bake_raw (src/world/importance_map.rs:78-253) over BOUNDED_VISIBLE_RANGE (parsing/environment.rs:140):
    // texel luminance = sum of 100 left-Riemann samples of luminance(lambda) * texel spectrum(lambda); per-row pdf and
    // cumulative mass over the columns, marginal over the rows.  Tables go to texture memory (HBM).
    bool bake_importance_map() {
        const pt_environment& e = d.environment;
        const uint32_t V = (uint32_t)e.importance_height, H = (uint32_t)e.importance_width;
        const int N = kVisibleSteps;
        float lum[N];
        ptd::SceneView view{w.data(), hs->tex.data()};
        for (int i = 0; i < N; ++i) {
            if (e.importance_luminance_curve >= 0) lum[i] = ptd::curve_eval(view, curve_off[e.importance_luminance_curve], visible_lambda(i));
            else { float xb, yb, zb; ptd::xyz_bar(visible_lambda(i) * 10.0f, &xb, &yb, &zb); lum[i] = yb; }
        }
        std::vector<float> row_pdf((size_t)V * H), row_cmf((size_t)V * H), mpdf(V), mcmf(V);
        // the spectral curves of the environment texture at the 100 wavelengths, evaluated once per channel instead of once
        // per texel (TexStack::eval_at re-evaluates them; same values)
        const pt_texstack& ets = d.texstacks[e.texstack];
        std::vector<float> cv((size_t)ets.layer_count * 4 * N, 0.0f);
        for (int li = 0; li < ets.layer_count; ++li) {
            const pt_texture_layer& L = d.layers[ets.first_layer + li];
            for (int c = 0; c < (L.kind == PT_TEXTURE4 ? 4 : 1); ++c)
                for (int i = 0; i < N; ++i) cv[((size_t)li * 4 + c) * N + i] = ptd::curve_eval(view, curve_off[L.curves[c]], visible_lambda(i));
        }
        float total = 0.0f;
        for (uint32_t row = 0; row < V; ++row) {
            float row_luminance = 0.0f;
            float* pdf = row_pdf.data() + (size_t)row * H; float* cmf = row_cmf.data() + (size_t)row * H;
            for (uint32_t col = 0; col < H; ++col) {
                float u = (float)row / (float)V, v = (float)col / (float)H;
                float cu = pt_clamp(u, 0.0f, 1.0f - PT_F32_EPSILON), cvv = pt_clamp(v, 0.0f, 1.0f - PT_F32_EPSILON);
                const float texel = visible_range_sum([&](int i) {
                    float energy = 0.0f;
                    for (int li = 0; li < ets.layer_count; ++li) {
                        const pt_texture_layer& L = d.layers[ets.first_layer + li];
                        const float* data = d.texture_data + L.data_offset;
                        size_t idx = (size_t)(cvv * (float)L.height) * (size_t)L.width + (size_t)(cu * (float)L.width);
                        const float* c = &cv[(size_t)li * 4 * N];
                        if (L.kind == PT_TEXTURE1) energy += c[i] * data[idx];
                        else { const float* t = data + 4 * idx; energy += (c[i] * t[0] + c[N + i] * t[1]) + (c[2 * N + i] * t[2] + c[3 * N + i] * t[3]); }
                    }
                    return lum[i] * energy;
                });
                row_luminance += texel;
                pdf[col] = texel; cmf[col] = row_luminance;
            }
            for (uint32_t col = 0; col < H; ++col) { pdf[col] /= row_luminance; cmf[col] /= row_luminance; }
            total += row_luminance;
            mpdf[row] = row_luminance;
        }
        float run = 0.0f;
        for (uint32_t row = 0; row < V; ++row) { mpdf[row] /= total; run += mpdf[row]; mcmf[row] = run; }
        if (hs->tex.size() + 2 * row_pdf.size() + 2 * (size_t)V + 64 > 0xffffffffull) return fail("importance map too large");
        w[PT_HDR_IMAP_ROWS] = V; w[PT_HDR_IMAP_COLS] = H;
        // pdf and cmf of a table interleaved, (cmf[k], pdf[k]): what a sample reads at its end lies on one line (pt_blob.h PT_HDR_IMAP_STRIDE);
        // the tables start on 128-byte lines (the texel array in front of them has any length)
        auto interleaved = [&](const std::vector<float>& cmf, const std::vector<float>& pdf, int cmf_hdr, int pdf_hdr) {
            while (hs->tex.size() % 32) hs->tex.push_back(0.0f);
            w[cmf_hdr] = (uint32_t)hs->tex.size(); w[pdf_hdr] = (uint32_t)hs->tex.size() + 1u;
            for (size_t k = 0; k < cmf.size(); ++k) { hs->tex.push_back(cmf[k]); hs->tex.push_back(pdf[k]); }
        };
        w[PT_HDR_IMAP_STRIDE] = 2u;
        interleaved(row_cmf, row_pdf, PT_HDR_IMAP_ROW_CMF, PT_HDR_IMAP_ROW_PDF);
        interleaved(mcmf, mpdf, PT_HDR_IMAP_MARG_CMF, PT_HDR_IMAP_MARG_PDF);
        // guide tables: entry j = lower bound of j / n in the cmf, so that a search starts in a bracket of a few entries
        // instead of at the whole table (ten dependent loads from L2/HBM per search otherwise)
        auto guide = [&](const float* cmf, uint32_t n) {
            uint32_t k = 0;
            for (uint32_t j = 0; j < n + 3; ++j) {
                if (j > n) k = n;
                else { float t = (float)j / (float)n; while (k < n && cmf[k] < t) ++k; }
                hs->tex.push_back(bits_f(k));
            }
        };
        w[PT_HDR_IMAP_MARG_GUIDE] = (uint32_t)hs->tex.size(); guide(mcmf.data(), V);
        w[PT_HDR_IMAP_ROW_GUIDE] = (uint32_t)hs->tex.size();
        for (uint32_t r = 0; r < V; ++r) guide(row_cmf.data() + (size_t)r * H, H);
        return true;
    }

    // ---- 11. the rest of the header: world radius (World::new, world/mod.rs:69-81), flags, sizes; the mesh section joins the core
    void finish_header() {
        float env_p = lights.empty() ? 1.0f : d.env_sampling_probability;
        w[PT_HDR_ENV_PROB] = fbits(env_p);
        float radius = 0.0f;
        if (d.instance_count) {
            Box wb = ibox[0]; for (uint32_t i = 1; i < d.instance_count; ++i) box_expand(wb, ibox[i]);
            float sx = wb.mx[0] - wb.mn[0], sy = wb.mx[1] - wb.mn[1], sz = wb.mx[2] - wb.mn[2];
            radius = std::sqrt(sx * sx + sy * sy + sz * sz) / 2.0f;
        }
        w[PT_HDR_WORLD_RADIUS] = fbits(radius);
        uint32_t flags = w[PT_HDR_FLAGS] & (PT_FLAG_SWEEP_WALKS | PT_FLAG_CONVEX);
        for (uint32_t i = 0; i < d.instance_count; ++i) {
            const pt_instance& in = d.instances[i];
            if (in.kind == PT_SHAPE_DISK) flags |= PT_FLAG_NO_TOP_CULL;
            // a mesh whose hits can carry a Light tag through its instance's material is not in the light list (world/mod.rs:45-54 only looks at
            // analytic instances' own ids and mesh face ids) but would pass pt.rs:178
            if (in.kind == PT_SHAPE_MESH && in.material != PT_MATERIAL_NONE && PT_MATERIAL_TAG(in.material) == PT_TAG_LIGHT) flags |= PT_FLAG_NO_SHADOW_BOUND;
        }
        w[PT_HDR_FLAGS] = flags;
        pad16(w);
        w[PT_HDR_CORE_WORDS] = (uint32_t)w.size();
        w.insert(w.end(), md.begin(), md.end());
        pad16(w);
        w[PT_HDR_MAGIC] = PT_BLOB_MAGIC; w[PT_HDR_TOTAL_WORDS] = (uint32_t)w.size();
        hs->light_count = (uint32_t)lights.size();
        hs->material_count = d.material_count;
        hs->curve_count = d.curve_count;
    }
};

}  // namespace

// The curves' cell tables are an accelerator, and a scene that fits the LDS whole without them and not with them is better off without (the kernels of a scene staged
// whole never touch global memory for scene data: G2F at 24.3 KB): built again without the tables then.
bool build_host_scene(const pt_scene_desc& d, HostScene* hs, std::string* err) {
    uint32_t table_words = 0;
    if (!SceneBuild(d, hs, err).run(true, &table_words)) return false;
    const size_t bytes = hs->blob.size() * 4;
    if (table_words != 0 && bytes > PT_BLOB_LDS_ALL_BYTES && bytes - 4u * table_words <= PT_BLOB_LDS_ALL_BYTES) {
        *hs = HostScene();
        return SceneBuild(d, hs, err).run(false, &table_words);
    }
    return true;
}

}  // namespace pth
