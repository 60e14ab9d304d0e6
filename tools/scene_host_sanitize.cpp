// scene_host_sanitize.cpp — a stand-alone host program for a sanitizer run of the scene build (csrc/pt_scene_host.cpp): it builds a handful of descriptions in heap
// arrays of exactly the sizes they name — analytic shapes under transforms, a cube mesh of two instances whose triangles the sweep table inlines, a closed
// sphere mesh of 160 faces with vertex normals that is walked (leaf list, group boxes, inner balls, slabs, convex certificate), and an HDR environment with a
// baked importance map, and a scene with no instance at all (the smallest blob) — so that a read past a description's array or a write past a blob's record
// is a heap overflow the sanitizer sees.  Over every scene built it then runs the engine's choice of kernel forms (csrc/pt_plan.cpp: plan_scene, plan_render) under
// four tunings, the PT_TUNE_NO_MESH_SHORTCUTS edit of the mesh records among them, each on a copy of the blob of its exact length.  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/scene_host_sanitize tools/scene_host_sanitize.cpp rust-pathtracer_amd/csrc/pt_scene_host.cpp rust-pathtracer_amd/csrc/pt_plan.cpp && /tmp/scene_host_sanitize
// It prints one line per description, one per tuning, and "ok" at the end; a refused description or a blob whose header does not name its own size ends it with status 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../rust-pathtracer_amd/csrc/pt_scene_host.h"

namespace {

struct Desc {   // a description's arrays, each a heap block of its exact length
    std::vector<pt_curve> curves; std::vector<float> curve_data;
    std::vector<pt_texture_layer> layers; std::vector<pt_texstack> texstacks; std::vector<float> texels;
    std::vector<pt_material> materials; std::vector<pt_mesh> meshes;
    std::vector<float> vertices, normals; std::vector<uint32_t> indices, face_materials;
    std::vector<pt_instance> instances; std::vector<pt_camera> cameras;
    pt_environment env;

    int32_t flat(float v) {   // a one-sample linear curve
        curves.push_back(pt_curve{PT_CURVE_LINEAR, PT_INTERP_LINEAR, 370.0f, 790.0f, (uint32_t)curve_data.size(), 1u});
        curve_data.push_back(v);
        return (int32_t)curves.size() - 1;
    }
    int32_t tabulated(int knots, float lo, float hi) {   // enough knots for a cell table
        curves.push_back(pt_curve{PT_CURVE_TABULATED, PT_INTERP_CUBIC, 0.0f, 0.0f, (uint32_t)curve_data.size(), (uint32_t)knots});
        for (int k = 0; k < knots; ++k) { curve_data.push_back(lo + (hi - lo) * (float)k / (float)(knots - 1)); curve_data.push_back(0.2f + 0.5f * (float)(k % 3)); }
        return (int32_t)curves.size() - 1;
    }
    uint32_t material(pt_material m, int tag) { materials.push_back(m); return PT_MATERIAL_ID(tag, materials.size() - 1); }

    Desc() {
        std::memset(&env, 0, sizeof(env));
        const int32_t zero = flat(0.0f), five = flat(5.0f);
        pt_material error; std::memset(&error, 0, sizeof(error));
        error.kind = PT_MATERIAL_DIFFUSE_LIGHT; error.curve_emit = five; error.curve_bounce = zero; error.sidedness = PT_SIDED_DUAL;
        material(error, PT_TAG_LIGHT);
        env.kind = PT_ENV_CONSTANT; env.curve = zero; env.strength = 0.0f;
        pt_camera cam; std::memset(&cam, 0, sizeof(cam));
        cam.look_from[0] = 4.0f; cam.v_up[2] = 1.0f; cam.vfov = 40.0f; cam.focal_distance = 4.0f;
        cameras.push_back(cam);
    }
    uint32_t lambertian(int32_t curve) {
        layers.push_back(pt_texture_layer{PT_TEXTURE1, {curve, -1, -1, -1}, 1, 1, (uint64_t)texels.size()});
        texels.push_back(1.0f);
        texstacks.push_back(pt_texstack{(int32_t)layers.size() - 1, 1});
        pt_material m; std::memset(&m, 0, sizeof(m));
        m.kind = PT_MATERIAL_LAMBERTIAN; m.texstack = (int32_t)texstacks.size() - 1;
        return material(m, PT_TAG_MATERIAL);
    }
    uint32_t glass() {
        pt_material m; std::memset(&m, 0, sizeof(m));
        m.kind = PT_MATERIAL_GGX; m.alpha = 0.05f; m.curve_eta = flat(1.5f); m.curve_eta_o = flat(1.0f); m.curve_kappa = tabulated(12, 380.0f, 750.0f);
        return material(m, PT_TAG_MATERIAL);
    }
    uint32_t lamp() {
        pt_material m; std::memset(&m, 0, sizeof(m));
        m.kind = PT_MATERIAL_DIFFUSE_LIGHT; m.curve_emit = flat(5.0f); m.curve_bounce = 0; m.sidedness = PT_SIDED_DUAL;
        return material(m, PT_TAG_LIGHT);
    }
    pt_instance& instance(int32_t kind, uint32_t mat) {
        pt_instance in; std::memset(&in, 0, sizeof(in));
        in.kind = kind; in.material = mat; in.mesh = -1;
        for (int k = 0; k < 4; ++k) { in.forward[5 * k] = 1.0f; in.reverse[5 * k] = 1.0f; }
        instances.push_back(in);
        return instances.back();
    }
    static void move_and_scale(pt_instance& in, float s, float x, float y, float z) {
        in.has_transform = 1;
        for (int k = 0; k < 3; ++k) { in.forward[5 * k] = s; in.reverse[5 * k] = 1.0f / s; }
        const float t[3] = {x, y, z};
        for (int k = 0; k < 3; ++k) { in.forward[4 * k + 3] = t[k]; in.reverse[4 * k + 3] = -t[k] / s; }
    }
    int32_t mesh(const std::vector<float>& p, const std::vector<uint32_t>& f, bool with_normals, uint32_t mat) {
        pt_mesh m{(uint32_t)(vertices.size() / 3), (uint32_t)(p.size() / 3), (uint32_t)indices.size(), (uint32_t)(f.size() / 3), -1, (int32_t)face_materials.size()};
        if (with_normals) {   // (of a body around the origin: the positions, normalised)
            m.normal_offset = (int32_t)(normals.size() / 3);
            for (size_t v = 0; v < p.size(); v += 3) {
                const float l = std::sqrt(p[v] * p[v] + p[v + 1] * p[v + 1] + p[v + 2] * p[v + 2]);
                for (int k = 0; k < 3; ++k) normals.push_back(p[v + k] / l);
            }
        }
        vertices.insert(vertices.end(), p.begin(), p.end()); indices.insert(indices.end(), f.begin(), f.end());
        face_materials.insert(face_materials.end(), f.size() / 3, mat);
        meshes.push_back(m);
        return (int32_t)meshes.size() - 1;
    }

    int build(const char* name) {
        auto exact = [](auto& v) { v.shrink_to_fit(); return v.empty() ? nullptr : v.data(); };
        pt_scene_desc d; std::memset(&d, 0, sizeof(d));
        d.curve_count = (uint32_t)curves.size(); d.curves = exact(curves); d.curve_data_count = curve_data.size(); d.curve_data = exact(curve_data);
        d.layer_count = (uint32_t)layers.size(); d.layers = exact(layers); d.texstack_count = (uint32_t)texstacks.size(); d.texstacks = exact(texstacks);
        d.texture_data_count = texels.size(); d.texture_data = exact(texels);
        d.material_count = (uint32_t)materials.size(); d.materials = exact(materials);
        d.mesh_count = (uint32_t)meshes.size(); d.meshes = exact(meshes);
        d.vertex_count = vertices.size() / 3; d.vertices = exact(vertices); d.index_count = indices.size(); d.indices = exact(indices);
        d.normal_count = normals.size() / 3; d.normals = exact(normals); d.face_material_count = face_materials.size(); d.face_materials = exact(face_materials);
        d.instance_count = (uint32_t)instances.size(); d.instances = exact(instances);
        d.camera_count = (uint32_t)cameras.size(); d.cameras = exact(cameras);
        d.environment = env; d.env_sampling_probability = 0.5f;
        pth::HostScene hs; std::string err;
        if (!pth::build_host_scene(d, &hs, &err)) { printf("FAILED: %s refused: %s\n", name, err.c_str()); return 1; }
        if (hs.blob[PT_HDR_MAGIC] != PT_BLOB_MAGIC || hs.blob[PT_HDR_TOTAL_WORDS] != hs.blob.size() || hs.blob[PT_HDR_CORE_WORDS] > hs.blob.size()) { printf("FAILED: %s: the header does not name the blob's size\n", name); return 1; }
        printf("%s: %zu blob words (%u core), %zu texel words, %u lights, sweep table %s\n", name, hs.blob.size(), hs.blob[PT_HDR_CORE_WORDS], hs.tex.size(), hs.light_count,
               hs.blob[PT_HDR_SWEEP_OFF] ? ((hs.blob[PT_HDR_FLAGS] & PT_FLAG_SWEEP_WALKS) ? "with a walked mesh" : "yes") : "no");
        return plans(name, hs);
    }

    // The engine's choice of kernel forms (csrc/pt_plan.cpp: plan_scene, plan_render) over the scene just built: per tuning a copy of the blob in a heap block of
    // its exact length, which plan_scene edits in place (NO_MESH_SHORTCUTS writes into the mesh records) and plan_render only reads, for five kinds of render.
    static int plans(const char* name, const pth::HostScene& hs) {
        const uint32_t tunings[] = {0u, PT_TUNE_NO_MESH_SHORTCUTS | PT_TUNE_NO_CONVEX, PT_TUNE_NO_SWEEP | PT_TUNE_NO_PARK, PT_TUNE_NO_LDS | PT_TUNE_GENERAL_FORMS};
        for (uint32_t flags : tunings) {
            pt_tuning tn; std::memset(&tn, 0, sizeof(tn));
            tn.flags = flags; tn.park_dynamic = -1;
            std::vector<uint32_t> blob(hs.blob);
            const pth::ScenePlan sp = pth::plan_scene(tn, blob);
            pt_render_desc in; std::memset(&in, 0, sizeof(in));
            in.width = 64; in.height = 48; in.spp = 10; in.min_bounces = 1; in.max_bounces = 6; in.light_samples = 2; in.wavelength_lo = 380.0f; in.wavelength_hi = 750.0f;
            const pt_adaptive_desc adaptive{40u, 20u, 0.05f, 0.0f};
            for (int kind = 0; kind < 5; ++kind) {   // plain, four wavelengths, medium-aware, adaptive, routed
                pth::RenderAsk ask;
                pt_render_desc rd = in;
                rd.hero_wavelengths = kind == 1 ? 4u : 1u; rd.medium_aware = kind == 2;
                std::string err;
                if (!pth::normalize_render_desc(rd, (uint32_t)hs.cameras.size(), &ask.rd, &err)) { printf("FAILED: %s: %s\n", name, err.c_str()); return 1; }
                ask.num_cus = 256; ask.n_pixels = (size_t)rd.width * rd.height; ask.adaptive = kind == 3 ? &adaptive : nullptr; ask.routed = kind == 4;
                pth::RenderPlan p;
                if (!pth::plan_render(blob, tn, sp, ask, &p, &err)) { printf("FAILED: %s: %s\n", name, err.c_str()); return 1; }
                if (kind == 0) printf("  tuning 0x%x: flags 0x%x, lacks %u, lds mode %d; traversal form %d, vertex form %d, %u slots\n", flags, blob[PT_HDR_FLAGS], sp.lacks, sp.lds_mode, p.trav_form, p.shade_form, p.capacity);
            }
        }
        return 0;
    }
};

const std::vector<float> kCube = {-0.5f, -0.5f, -0.5f, 0.5f, -0.5f, -0.5f, 0.5f, 0.5f, -0.5f, -0.5f, 0.5f, -0.5f, -0.5f, -0.5f, 0.5f, 0.5f, -0.5f, 0.5f, 0.5f, 0.5f, 0.5f, -0.5f, 0.5f, 0.5f};
const std::vector<uint32_t> kCubeFaces = {0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 1, 2, 6, 1, 6, 5, 2, 3, 7, 2, 7, 6, 3, 0, 4, 3, 4, 7};

void room(Desc& s) {   // a floor and a lamp
    const uint32_t white = s.lambertian(s.tabulated(20, 380.0f, 750.0f));
    pt_instance& floor = s.instance(PT_SHAPE_RECT, white); floor.size[0] = 8.0f; floor.size[1] = 8.0f; floor.origin[2] = -1.5f; floor.axis = PT_AXIS_Z; floor.two_sided = 1;
    pt_instance& light = s.instance(PT_SHAPE_RECT, s.lamp()); light.size[0] = 1.0f; light.size[1] = 1.0f; light.origin[2] = 3.0f; light.axis = PT_AXIS_Z; light.two_sided = 1;
}

int analytic_shapes() {
    Desc s; room(s);
    const uint32_t glass = s.glass();
    pt_instance& ball = s.instance(PT_SHAPE_SPHERE, glass); ball.radius = 0.4f; ball.origin[0] = 1.0f;
    pt_instance& ball2 = s.instance(PT_SHAPE_SPHERE, glass); ball2.radius = 0.3f; Desc::move_and_scale(ball2, 1.5f, -1.0f, 0.5f, 0.0f);
    pt_instance& disk = s.instance(PT_SHAPE_DISK, s.lamp()); disk.radius = 0.5f; disk.origin[1] = 1.0f; disk.two_sided = 1; Desc::move_and_scale(disk, 0.7f, 0.0f, 1.0f, 1.0f);
    pt_instance& wall = s.instance(PT_SHAPE_RECT, glass); wall.size[0] = 1.0f; wall.size[1] = 2.0f; wall.origin[0] = -2.0f; wall.axis = PT_AXIS_X;
    return s.build("analytic shapes");
}

int inlined_mesh() {
    Desc s; room(s);
    const int32_t cube = s.mesh(kCube, kCubeFaces, false, PT_MATERIAL_ID(PT_TAG_MATERIAL, 1));
    s.instance(PT_SHAPE_MESH, PT_MATERIAL_NONE).mesh = cube;
    pt_instance& second = s.instance(PT_SHAPE_MESH, s.glass()); second.mesh = cube; Desc::move_and_scale(second, 0.6f, 1.2f, 0.0f, 0.0f);
    pt_instance& lamp = s.instance(PT_SHAPE_SPHERE, s.lamp()); lamp.radius = 0.05f; lamp.origin[0] = 1.2f;   // (inside the second cube's box: it is certified outward only)
    return s.build("inlined mesh");
}

int walked_mesh(bool emissive) {
    Desc s; room(s);
    const int rings = 9, around = 10;   // a closed sphere: 2 * around * (rings - 1) = 160 faces
    std::vector<float> p = {0.0f, 0.0f, 1.0f};
    for (int r = 1; r < rings; ++r)
        for (int a = 0; a < around; ++a) {
            const double th = M_PI * r / rings, ph = 2.0 * M_PI * a / around;
            p.push_back((float)(std::sin(th) * std::cos(ph))); p.push_back((float)(std::sin(th) * std::sin(ph))); p.push_back((float)std::cos(th));
        }
    p.insert(p.end(), {0.0f, 0.0f, -1.0f});
    const uint32_t south = 1 + (rings - 1) * around;
    std::vector<uint32_t> f;
    auto at = [&](int r, int a) { return (uint32_t)(1 + (r - 1) * around + a % around); };
    for (int a = 0; a < around; ++a) {
        f.insert(f.end(), {0u, at(1, a), at(1, a + 1)});
        for (int r = 1; r < rings - 1; ++r) { f.insert(f.end(), {at(r, a), at(r + 1, a), at(r + 1, a + 1)}); f.insert(f.end(), {at(r, a), at(r + 1, a + 1), at(r, a + 1)}); }
        f.insert(f.end(), {south, at(rings - 1, a + 1), at(rings - 1, a)});
    }
    const uint32_t skin = emissive ? s.lamp() : s.glass();
    const int32_t ball = s.mesh(p, f, true, emissive ? skin : PT_MATERIAL_ID(PT_TAG_MATERIAL, 1));
    pt_instance& in = s.instance(PT_SHAPE_MESH, emissive ? PT_MATERIAL_NONE : skin); in.mesh = ball; Desc::move_and_scale(in, 0.8f, 0.0f, 0.0f, 0.2f);
    return s.build(emissive ? "walked mesh of emissive faces" : "walked mesh");
}

int hdr_environment() {
    Desc s; room(s);
    const int W = 8, H = 4;
    const int32_t r = s.tabulated(30, 380.0f, 750.0f), g = s.tabulated(9, 400.0f, 700.0f), b = s.flat(0.3f), zero = 0;
    s.layers.push_back(pt_texture_layer{PT_TEXTURE4, {r, g, b, zero}, W, H, (uint64_t)s.texels.size()});
    for (int k = 0; k < W * H; ++k) { s.texels.push_back(0.1f + 0.05f * (float)k); s.texels.push_back(0.5f); s.texels.push_back(1.0f / (float)(k + 1)); s.texels.push_back(1.0f); }
    s.texstacks.push_back(pt_texstack{(int32_t)s.layers.size() - 1, 1});
    s.env.kind = PT_ENV_HDR; s.env.curve = -1; s.env.strength = 1.0f; s.env.texstack = (int32_t)s.texstacks.size() - 1;
    for (int k = 0; k < 4; ++k) { s.env.rotation_forward[5 * k] = 1.0f; s.env.rotation_reverse[5 * k] = 1.0f; }
    s.env.importance_width = 7; s.env.importance_height = 5; s.env.importance_luminance_curve = -1;
    return s.build("hdr environment with an importance map");
}

int no_instance() {   // the smallest blob: an environment and a camera
    Desc s;
    return s.build("no instance at all");
}

}  // namespace

int main() {
    if (no_instance() || analytic_shapes() || inlined_mesh() || walked_mesh(false) || walked_mesh(true) || hdr_environment()) return 1;
    printf("ok\n");
    return 0;
}
