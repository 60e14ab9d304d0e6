// scene_file.cpp — config / scene / library TOML files -> pt_scene_desc, pt_render_desc, pt_output_desc.
// See include/pt_scene_file.h for the reference functions this restates.  CPU-only (libptscene.so).
#include "../../../include/pt_scene_file.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "image_io.h"
#include "obj_io.h"
#include "toml_lite.h"

namespace {

thread_local std::string g_error;
std::string g_root;

struct Failure { pt_status status; std::string message; };
[[noreturn]] void fail(const std::string& m, pt_status st = PT_ERR_INVALID_ARGUMENT) { throw Failure{st, m}; }

std::string resolve_path(const std::string& p) {
    if (std::ifstream(p).good() || g_root.empty() || (!p.empty() && p[0] == '/')) return p;
    std::string q = g_root + (g_root.back() == '/' ? "" : "/") + p;
    return std::ifstream(q).good() ? q : p;
}
std::string read_text(const std::string& path) {
    std::ifstream f(resolve_path(path), std::ios::binary);
    if (!f) fail("failed to load file " + path);
    std::ostringstream ss; ss << f.rdbuf();
    return ss.str();
}
toml::Value parse_file(const std::string& path) {
    try { return toml::parse(read_text(path)); }
    catch (const toml::ParseError& e) { fail("failed to parse " + path + ": " + e.what()); }
}

// ---- serde-like field access with deny_unknown_fields -------------------------------------------------------------
class Fields {
public:
    Fields(const toml::Value& v, std::string context) : ctx_(std::move(context)) {
        if (v.kind != toml::Value::TableKind) fail(ctx_ + ": expected a table");
        t_ = v.t.get();
    }
    const toml::Value* opt(const std::string& key) { seen_.insert(key); return t_->find(key); }
    const toml::Value& req(const std::string& key) { const toml::Value* v = opt(key); if (!v) fail(ctx_ + ": missing field `" + key + "`"); return *v; }
    std::string str(const std::string& key) { const toml::Value& v = req(key); if (v.kind != toml::Value::String) fail(ctx_ + "." + key + ": expected a string"); return v.s; }
    bool has(const std::string& key) { return opt(key) != nullptr; }
    float f32(const std::string& key) { return num(req(key), key); }
    float f32_or(const std::string& key, float d) { const toml::Value* v = opt(key); return v ? num(*v, key) : d; }
    int64_t integer(const std::string& key, int64_t lo, int64_t hi) { return integer_of(req(key), key, lo, hi); }
    int64_t integer_or(const std::string& key, int64_t lo, int64_t hi, int64_t d) { const toml::Value* v = opt(key); return v ? integer_of(*v, key, lo, hi) : d; }
    bool boolean(const std::string& key) { const toml::Value& v = req(key); if (v.kind != toml::Value::Boolean) fail(ctx_ + "." + key + ": expected a boolean"); return v.b; }
    int tri_bool(const std::string& key) { const toml::Value* v = opt(key); if (!v) return -1; if (v->kind != toml::Value::Boolean) fail(ctx_ + "." + key + ": expected a boolean"); return v->b ? 1 : 0; }
    void floats(const std::string& key, float* out, size_t n) { floats_of(req(key), key, out, n); }
    bool floats_opt(const std::string& key, float* out, size_t n) { const toml::Value* v = opt(key); if (!v) return false; floats_of(*v, key, out, n); return true; }
    void done() { for (auto& kv : t_->items) if (!seen_.count(kv.first)) fail(ctx_ + ": unknown field `" + kv.first + "`"); }
    const std::string& context() const { return ctx_; }

private:
    float num(const toml::Value& v, const std::string& key) { if (!v.is_number()) fail(ctx_ + "." + key + ": expected a number"); return (float)v.number(); }
    int64_t integer_of(const toml::Value& v, const std::string& key, int64_t lo, int64_t hi) {
        if (v.kind != toml::Value::Integer || v.i < lo || v.i > hi) fail(ctx_ + "." + key + ": expected an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
        return v.i;
    }
    void floats_of(const toml::Value& v, const std::string& key, float* out, size_t n) {
        if (v.kind != toml::Value::ArrayKind || v.a->size() != n) fail(ctx_ + "." + key + ": expected an array of " + std::to_string(n) + " numbers");
        for (size_t k = 0; k < n; ++k) out[k] = num((*v.a)[k], key);
    }
    const toml::Table* t_;
    std::string ctx_;
    std::set<std::string> seen_;
};

int enum_of(const std::string& value, std::initializer_list<const char*> names, const std::string& ctx) {
    int k = 0;
    for (const char* n : names) { if (value == n) return k; ++k; }
    fail(ctx + ": unknown variant `" + value + "`");
}

// ---- Transform3 (math crate), in f64 like rust-pathtracer_amd/scene.py so that both front ends agree bit for bit --------
struct Mat4 { double m[4][4]; };
Mat4 identity() { Mat4 r; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) r.m[i][j] = i == j ? 1.0 : 0.0; return r; }
Mat4 mul(const Mat4& a, const Mat4& b) {
    Mat4 r;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double s = 0.0; for (int k = 0; k < 4; ++k) s += a.m[i][k] * b.m[k][j]; r.m[i][j] = s; }
    return r;
}
Mat4 inverse(const Mat4& src) {  // Gauss-Jordan with partial pivoting (first largest pivot); same operation order as scene.py
    Mat4 a = src, inv = identity();
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(a.m[r][col]) > std::fabs(a.m[piv][col])) piv = r;
        if (a.m[piv][col] == 0.0) fail("singular transform");
        if (piv != col) for (int j = 0; j < 4; ++j) { std::swap(a.m[piv][j], a.m[col][j]); std::swap(inv.m[piv][j], inv.m[col][j]); }
        double p = a.m[col][col];
        for (int j = 0; j < 4; ++j) { a.m[col][j] /= p; inv.m[col][j] /= p; }
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            double f = a.m[r][col];
            for (int j = 0; j < 4; ++j) { a.m[r][j] -= f * a.m[col][j]; inv.m[r][j] -= f * inv.m[col][j]; }
        }
    }
    return inv;
}
struct AxisAngle { float axis[3]; float angle; };
Mat4 from_axis_angle(const float* axis, double angle_rad) {
    double x = axis[0], y = axis[1], z = axis[2], n = std::sqrt(x * x + y * y + z * z);
    x /= n; y /= n; z /= n;
    double c = std::cos(angle_rad), s = std::sin(angle_rad);
    Mat4 r = identity();
    r.m[0][0] = c + x * x * (1 - c); r.m[0][1] = x * y * (1 - c) - z * s; r.m[0][2] = x * z * (1 - c) + y * s;
    r.m[1][0] = y * x * (1 - c) + z * s; r.m[1][1] = c + y * y * (1 - c); r.m[1][2] = y * z * (1 - c) - x * s;
    r.m[2][0] = z * x * (1 - c) - y * s; r.m[2][1] = z * y * (1 - c) + x * s; r.m[2][2] = c + z * z * (1 - c);
    return r;
}
// Transform3Data -> Transform3 (src/parsing/instance.rs:40-71): from_stack(scale, rotate, translate) = T * R * S,
// rotations applied in list order (each multiplies the accumulated rotation from the left)
Mat4 from_stack(const float* scale, const std::vector<AxisAngle>& rotate, const float* translate) {
    Mat4 m = identity();
    if (scale) { Mat4 s = identity(); for (int k = 0; k < 3; ++k) s.m[k][k] = scale[k]; m = mul(s, m); }
    if (!rotate.empty()) {
        Mat4 base = identity(); bool first = true;
        for (auto& r : rotate) {
            Mat4 t = from_axis_angle(r.axis, 3.141592653589793 * (double)r.angle / 180.0);
            base = first ? t : mul(t, base); first = false;
        }
        m = mul(base, m);
    }
    if (translate) { Mat4 t = identity(); for (int k = 0; k < 3; ++k) t.m[k][3] = translate[k]; m = mul(t, m); }
    return m;
}
void store(const Mat4& m, float* out) { for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = (float)m.m[i][j]; }
std::vector<AxisAngle> parse_rotations(const toml::Value& v, const std::string& ctx) {
    if (v.kind != toml::Value::ArrayKind) fail(ctx + ": expected an array of {axis, angle}");
    std::vector<AxisAngle> out;
    for (auto& e : *v.a) { Fields f(e, ctx); AxisAngle a; f.floats("axis", a.axis, 3); a.angle = f.f32("angle"); f.done(); out.push_back(a); }
    return out;
}

// ---- curves (src/parsing/curves.rs) ----------------------------------------------------------------------------------
struct CurveM { int kind = 0, mode = 0; float p0 = 0, p1 = 0; std::vector<float> data; uint32_t count = 0; };

bool parse_f32(const std::string& s, float* out) {  // str::trim().parse::<f32>()
    size_t b = s.find_first_not_of(" \t\r\n"), e = s.find_last_not_of(" \t\r\n");
    if (b == std::string::npos) return false;
    std::string t = s.substr(b, e - b + 1);
    if (t.find_first_of("xX") != std::string::npos) return false;
    char* end = nullptr;
    float v = std::strtof(t.c_str(), &end);
    if (end == t.c_str() || *end) return false;
    *out = v;
    return true;
}
struct DomainMapping { float x_offset = 0, x_scale = 1, y_offset = 0, y_scale = 1; };
DomainMapping parse_domain_mapping(const toml::Value* v, const std::string& ctx) {
    DomainMapping d;
    if (!v) return d;
    Fields f(*v, ctx + ".domain_mapping");
    d.x_offset = f.f32_or("x_offset", 0.0f); d.x_scale = f.f32_or("x_scale", 1.0f);
    d.y_offset = f.f32_or("y_offset", 0.0f); d.y_scale = f.f32_or("y_scale", 1.0f);
    f.done();
    return d;
}
int interpolation_mode(Fields& f) { return enum_of(f.str("interpolation_mode"), {"Linear", "Nearest", "Cubic"}, f.context() + ".interpolation_mode"); }

// parse_tabulated_curve_from_csv (curves.rs:137-173): x = first column, y = column `column`; unparsable lines are skipped
CurveM tabulated_from_csv(const std::string& text, size_t column, int mode, const DomainMapping& dm) {
    if (column == 0) fail("TabulatedCSV: column must be > 0");
    CurveM c; c.kind = PT_CURVE_TABULATED; c.mode = mode;
    size_t p = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        std::string line = text.substr(p, e == std::string::npos ? std::string::npos : e - p);
        p = e == std::string::npos ? text.size() : e + 1;
        std::vector<std::string> cells;
        size_t q = 0;
        while (cells.size() < column + 1) {
            size_t k = line.find(',', q);
            cells.push_back(line.substr(q, k == std::string::npos ? std::string::npos : k - q));
            if (k == std::string::npos) break;
            q = k + 1;
        }
        if (cells.size() < column + 1) continue;
        float x, y;
        if (!parse_f32(cells[0], &x) || !parse_f32(cells[column], &y)) continue;
        c.data.push_back((x - dm.x_offset) * dm.x_scale);
        c.data.push_back((y - dm.y_offset) * dm.y_scale);
    }
    c.count = (uint32_t)(c.data.size() / 2);
    return c;
}
// parse_linear (curves.rs:175-213): first line "start_x, step", then one value per line
CurveM linear_from_text(const std::string& text, int mode, const DomainMapping& dm, const std::string& name) {
    std::vector<std::string> lines;
    size_t p = 0;
    while (p < text.size()) { size_t e = text.find('\n', p); lines.push_back(text.substr(p, e == std::string::npos ? std::string::npos : e - p)); p = e == std::string::npos ? text.size() : e + 1; }
    if (lines.empty()) fail("loading linear data failed: " + name + " is empty");
    size_t comma = lines[0].find(',');
    float start, step;
    if (comma == std::string::npos || !parse_f32(lines[0].substr(0, comma), &start)) fail("loading linear data failed: " + name);
    std::string rest = lines[0].substr(comma + 1);
    size_t c2 = rest.find(',');
    if (!parse_f32(c2 == std::string::npos ? rest : rest.substr(0, c2), &step)) fail("loading linear data failed: " + name);
    CurveM c; c.kind = PT_CURVE_LINEAR; c.mode = mode;
    for (size_t k = 1; k < lines.size(); ++k) {
        float v;
        if (!parse_f32(lines[k], &v)) fail("loading linear data failed: " + name + " line " + std::to_string(k + 1));
        c.data.push_back((v - dm.y_offset) * dm.y_scale);
    }
    float end = start + step * (float)c.data.size();
    c.p0 = (start - dm.x_offset) * dm.x_scale; c.p1 = (end - dm.x_offset) * dm.x_scale;
    c.count = (uint32_t)c.data.size();
    return c;
}
CurveM flat_curve(float strength) {  // CurveData::Flat -> Curve::Linear over EXTENDED_VISIBLE_RANGE (curves.rs:354-358)
    CurveM c; c.kind = PT_CURVE_LINEAR; c.mode = PT_INTERP_LINEAR; c.p0 = 370.0f; c.p1 = 790.0f; c.data = {strength}; c.count = 1;
    return c;
}
CurveM curve_from_data(const toml::Value& v, const std::string& ctx) {  // impl From<CurveData> for Curve (curves.rs:298-372)
    Fields f(v, ctx);
    std::string type = f.str("type");
    CurveM c;
    if (type == "Blackbody") { c.kind = PT_CURVE_BLACKBODY; c.p0 = f.f32("temperature"); c.p1 = f.f32("strength"); }
    else if (type == "Linear") {
        std::string filename = f.str("filename");
        DomainMapping dm = parse_domain_mapping(f.opt("domain_mapping"), ctx);
        c = linear_from_text(read_text(filename), interpolation_mode(f), dm, filename);
    } else if (type == "TabulatedCSV") {
        std::string filename = f.str("filename");
        size_t column = (size_t)f.integer("column", 0, 1 << 20);
        DomainMapping dm = parse_domain_mapping(f.opt("domain_mapping"), ctx);
        c = tabulated_from_csv(read_text(filename), column, interpolation_mode(f), dm);
    } else if (type == "Flat") c = flat_curve(f.f32("strength"));
    else if (type == "Cauchy") { c.kind = PT_CURVE_CAUCHY; c.p0 = f.f32("a"); c.p1 = f.f32("b"); }
    else if (type == "SimpleSpike") {
        c.kind = PT_CURVE_EXPONENTIAL;
        float lambda = f.f32("lambda"), l = f.f32("left_taper"), r = f.f32("right_taper"), s = f.f32("strength");
        c.data = {lambda, l, r, s}; c.count = 1;
    } else fail(ctx + ": unknown variant `" + type + "`");
    f.done();
    return c;
}

// ---- the loaded scene ------------------------------------------------------------------------------------------------
struct Lib {  // Maybe*Lib (src/parsing/mod.rs:56-86): a literal table or the path of a TOML file holding one
    toml::Value root;
    const toml::Table* table() const { return root.t.get(); }
};
Lib resolve_lib(const toml::Value& v, const std::string& what) {
    Lib l;
    if (v.kind == toml::Value::String) l.root = parse_file(v.s);
    else if (v.kind == toml::Value::TableKind) l.root = v;
    else fail(what + ": expected a table or a file name");
    return l;
}

}  // namespace

struct pt_config {
    std::string scene_file;
    int renderer = PT_RENDERER_TILED;
    uint32_t tile_w = 0, tile_h = 0;
    bool has_env_prob = false; float env_prob = 0.5f;
    struct Settings { pt_render_settings s; std::string filename, camera_id; bool has_filename = false; };
    std::vector<std::unique_ptr<Settings>> settings;
};

struct pt_scene_file {
    std::vector<pt_curve> curves; std::vector<float> curve_data;
    std::vector<pt_texture_layer> layers; std::vector<pt_texstack> texstacks; std::vector<float> texture_data;
    std::vector<pt_material> materials;
    std::vector<pt_medium> mediums; std::map<std::string, int> medium_ids;   // MediumId = position in the library + 1 (0 = vacuum)
    std::vector<pt_mesh> meshes; std::vector<float> vertices; std::vector<uint32_t> indices; std::vector<float> normals; std::vector<uint32_t> face_materials;
    std::vector<pt_instance> instances;
    std::vector<pt_camera> cameras;
    pt_scene_desc desc;
    std::map<std::string, int> curve_names, texture_names, camera_names;
    std::map<std::string, uint32_t> material_ids;
    std::vector<std::string> warnings;
    // pt_scene_file_library_curve: the curves library the scene was loaded with, kept alive, and the curves resolved from it on request.  They live beside the
    // scene's own (curves, curve_data above are untouched: the pt_scene_desc is what it is without them).
    Lib curves_library;
    std::map<std::string, CurveM> library_curves;

    int add_curve(const CurveM& c) {
        pt_curve r; r.kind = c.kind; r.mode = c.mode; r.p0 = c.p0; r.p1 = c.p1; r.data_offset = (uint32_t)curve_data.size(); r.data_count = c.count;
        curve_data.insert(curve_data.end(), c.data.begin(), c.data.end());
        curves.push_back(r);
        return (int)curves.size() - 1;
    }
    void warn(const std::string& m) { warnings.push_back(m); }
};

namespace {

struct Loader {
    pt_scene_file& sf;
    const pt_config* config;
    Lib curves_lib, textures_lib, materials_lib, meshes_lib;

    // CurveDataOrReference::resolve (curves.rs:381-393): a literal becomes a fresh curve, a name refers to the library
    int curve_ref(const toml::Value& v, const std::string& ctx, bool* ok = nullptr) {
        if (v.kind == toml::Value::String) {
            auto it = sf.curve_names.find(v.s);
            if (it != sf.curve_names.end()) return it->second;
            const toml::Value* data = curves_lib.table()->find(v.s);
            if (!data) { if (ok) { *ok = false; return -1; } fail(ctx + ": curve `" + v.s + "` not found in the curves library"); }
            int idx = sf.add_curve(curve_from_data(*data, "curves." + v.s));
            sf.curve_names[v.s] = idx;
            return idx;
        }
        return sf.add_curve(curve_from_data(v, ctx));
    }

    // parse_texture_stack (texture.rs:155-326)
    int texture_stack(const std::string& name) {
        auto it = sf.texture_names.find(name);
        if (it != sf.texture_names.end()) return it->second;
        const toml::Value* v = textures_lib.table()->find(name);
        if (!v) return -1;
        if (v->kind != toml::Value::ArrayKind) fail("textures." + name + ": expected an array of texture layers");
        pt_texstack ts; ts.first_layer = (int32_t)sf.layers.size(); ts.layer_count = 0;
        std::vector<pt_texture_layer> layers;
        for (auto& lv : *v->a) {
            std::string ctx = "textures." + name;
            Fields f(lv, ctx);
            std::string type = f.str("type"), filename = f.str("filename"), err;
            pt_texture_layer layer; memset(&layer, 0, sizeof(layer));
            for (int k = 0; k < 4; ++k) layer.curves[k] = -1;
            pth::Image img;
            if (type == "Texture1") {
                layer.kind = PT_TEXTURE1;
                layer.curves[0] = curve_ref(f.req("curve"), ctx + ".curve");
                if (!pth::read_grey8(resolve_path(filename), &img, &err)) fail(ctx + ": " + err);
            } else if (type == "Texture4" || type == "HDR" || type == "EXR") {
                layer.kind = PT_TEXTURE4;
                const toml::Value& cs = f.req("curves");
                if (cs.kind != toml::Value::ArrayKind || cs.a->size() != 4) fail(ctx + ".curves: expected 4 curves");
                for (int k = 0; k < 4; ++k) layer.curves[k] = curve_ref((*cs.a)[k], ctx + ".curves");
                bool ok = type == "Texture4" ? pth::read_rgba8(resolve_path(filename), &img, &err)
                        : type == "HDR" ? pth::read_hdr(resolve_path(filename), f.f32_or("alpha_fill", 0.0f), &img, &err)
                                        : pth::read_exr(resolve_path(filename), &img, &err);
                if (!ok) fail(ctx + ": " + err);
            } else if (type == "SRGB") {  // texture.rs:283-318: the basis curves come from a fixed file
                layer.kind = PT_TEXTURE4;
                const std::string basis = "data/curves/basis/simple-spectral-srgb-1931.csv";
                std::string text = read_text(basis);
                for (int k = 0; k < 3; ++k) layer.curves[k] = sf.add_curve(tabulated_from_csv(text, (size_t)k + 1, PT_INTERP_CUBIC, DomainMapping()));
                layer.curves[3] = sf.add_curve(flat_curve(0.0f));
                if (!pth::read_rgba8(resolve_path(filename), &img, &err)) fail(ctx + ": " + err);
            } else fail(ctx + ": unknown variant `" + type + "`");
            f.done();
            layer.width = (int32_t)img.width; layer.height = (int32_t)img.height; layer.data_offset = sf.texture_data.size();
            sf.texture_data.insert(sf.texture_data.end(), img.data.begin(), img.data.end());
            layers.push_back(layer);
        }
        ts.first_layer = (int32_t)sf.layers.size(); ts.layer_count = (int32_t)layers.size();
        sf.layers.insert(sf.layers.end(), layers.begin(), layers.end());
        sf.texstacks.push_back(ts);
        sf.texture_names[name] = (int)sf.texstacks.size() - 1;
        return (int)sf.texstacks.size() - 1;
    }

    // MaterialData::resolve (material.rs:66-153) + id assignment (mod.rs:456-467); false = "failed to parse material"
    bool material(const std::string& name, const toml::Value& v) {
        std::string ctx = "materials." + name;
        Fields f(v, ctx);
        std::string type = f.str("type");
        pt_material m; memset(&m, 0, sizeof(m));
        m.texstack = m.curve_eta = m.curve_eta_o = m.curve_kappa = m.curve_emit = m.curve_bounce = -1;
        bool light = false, ok = true;
        if (type == "Lambertian") {
            m.kind = PT_MATERIAL_LAMBERTIAN;
            std::string tex = f.str("texture_id");
            m.texstack = texture_stack(tex);
            if (m.texstack < 0) fail(ctx + ": didn't find texture stack id for texture name " + tex);
        } else if (type == "GGX") {
            m.kind = PT_MATERIAL_GGX;
            m.alpha = f.f32("alpha");
            m.curve_eta = curve_ref(f.req("eta"), ctx + ".eta", &ok);
            if (ok) m.curve_eta_o = curve_ref(f.req("eta_o"), ctx + ".eta_o", &ok); else f.req("eta_o");
            if (ok) m.curve_kappa = curve_ref(f.req("kappa"), ctx + ".kappa", &ok); else f.req("kappa");
            f.f32("permeability");
            // material.rs:86-91: an unknown or missing name is the vacuum
            auto medium_of = [&](const char* key) { const toml::Value* v2 = f.opt(key); if (!v2) return 0; if (v2->kind != toml::Value::String) fail(ctx + "." + key + ": expected a string");
                                                    auto it = sf.medium_ids.find(v2->s); return it == sf.medium_ids.end() ? 0 : it->second; };
            m.outer_medium = medium_of("outer_medium_id"); m.inner_medium = medium_of("inner_medium_id");
        } else if (type == "DiffuseLight" || type == "SharpLight") {
            light = true;
            m.kind = type == "DiffuseLight" ? PT_MATERIAL_DIFFUSE_LIGHT : PT_MATERIAL_SHARP_LIGHT;
            m.curve_emit = curve_ref(f.req("emit_color"), ctx + ".emit_color", &ok);
            if (ok) m.curve_bounce = curve_ref(f.req("bounce_color"), ctx + ".bounce_color", &ok); else f.req("bounce_color");
            m.sidedness = enum_of(f.str("sidedness"), {"Forward", "Reverse", "Dual"}, ctx + ".sidedness");
            if (type == "SharpLight") m.sharpness = f.f32("sharpness");
        } else fail(ctx + ": unknown variant `" + type + "`");
        f.done();
        if (!ok) { sf.warn("failed to parse material " + name); return false; }
        sf.materials.push_back(m);
        sf.material_ids[name] = PT_MATERIAL_ID(light ? PT_TAG_LIGHT : PT_TAG_MATERIAL, sf.materials.size() - 1);
        return true;
    }
};

void build_desc(pt_scene_file& sf) {
    pt_scene_desc& d = sf.desc;
    d.curve_count = (uint32_t)sf.curves.size(); d.curves = sf.curves.data();
    d.curve_data_count = sf.curve_data.size(); d.curve_data = sf.curve_data.data();
    d.layer_count = (uint32_t)sf.layers.size(); d.layers = sf.layers.data();
    d.texstack_count = (uint32_t)sf.texstacks.size(); d.texstacks = sf.texstacks.data();
    d.texture_data_count = sf.texture_data.size(); d.texture_data = sf.texture_data.data();
    d.material_count = (uint32_t)sf.materials.size(); d.materials = sf.materials.data();
    d.mesh_count = (uint32_t)sf.meshes.size(); d.meshes = sf.meshes.data();
    d.vertex_count = sf.vertices.size() / 3; d.vertices = sf.vertices.data();
    d.index_count = sf.indices.size(); d.indices = sf.indices.data();
    d.normal_count = sf.normals.size() / 3; d.normals = sf.normals.data();
    d.face_material_count = sf.face_materials.size(); d.face_materials = sf.face_materials.data();
    d.instance_count = (uint32_t)sf.instances.size(); d.instances = sf.instances.data();
    d.camera_count = (uint32_t)sf.cameras.size(); d.cameras = sf.cameras.data();
    d.medium_count = (uint32_t)sf.mediums.size(); d.mediums = sf.mediums.empty() ? nullptr : sf.mediums.data();
}

void load_scene(const std::string& path, const pt_config* config, pt_scene_file& sf) {
    toml::Value root = parse_file(path);
    Fields top(root, path);
    memset(&sf.desc, 0, sizeof(sf.desc));
    Loader L{sf, config, resolve_lib(top.req("curves"), "curves"), resolve_lib(top.req("textures"), "textures"),
             resolve_lib(top.req("materials"), "materials"), resolve_lib(top.req("meshes"), "meshes")};
    sf.curves_library = L.curves_lib;
    // mediums (mod.rs:389-419, medium.rs): every entry of the library, in file order.  The reference numbers them from 0 in HashMap order while
    // its walk reads id 0 as the vacuum and id k as mediums[k - 1] (utils.rs:768-770), so a material there tracks the medium BEFORE the one
    // it names; here a name means its own medium: id = position + 1.
    std::vector<std::pair<std::string, toml::Value>> medium_entries;
    if (const toml::Value* mv = top.opt("mediums")) { Lib ml = resolve_lib(*mv, "mediums"); medium_entries = ml.table()->items; }
    sf.desc.env_sampling_probability = top.f32_or("env_sampling_probability", 0.5f);  // mod.rs:559
    const toml::Value& instances = top.req("instances");
    const toml::Value& cameras = top.req("cameras");
    const toml::Value& env = top.req("environment");
    top.done();
    if (instances.kind != toml::Value::ArrayKind || cameras.kind != toml::Value::ArrayKind) fail(path + ": instances and cameras must be arrays of tables");

    // material 0 = the mauve error light (mod.rs:438-455; src/curves.rs:41-48)
    {
        CurveM mauve; mauve.kind = PT_CURVE_EXPONENTIAL; mauve.data = {650.0f, 300.0f, 300.0f, 1.0f, 460.0f, 200.0f, 400.0f, 0.75f}; mauve.count = 2;
        pt_material m; memset(&m, 0, sizeof(m));
        m.kind = PT_MATERIAL_DIFFUSE_LIGHT; m.texstack = m.curve_eta = m.curve_eta_o = m.curve_kappa = -1;
        m.curve_emit = sf.add_curve(mauve); m.curve_bounce = sf.add_curve(flat_curve(0.0f)); m.sidedness = PT_SIDED_DUAL;
        sf.curve_names["__mauve"] = m.curve_emit;
        sf.materials.push_back(m);
        sf.material_ids["error"] = PT_MATERIAL_ID(PT_TAG_LIGHT, 0);
    }

    for (auto& kv : medium_entries) {
        const std::string ctx = "mediums." + kv.first;
        Fields f(kv.second, ctx);
        const std::string type = f.str("type");
        pt_medium m; memset(&m, 0, sizeof(m));
        m.curve_g = m.curve_sigma_a = m.curve_sigma_s = m.curve_ior = -1;
        if (type == "HG") {
            m.kind = PT_MEDIUM_HG;
            m.curve_g = L.curve_ref(f.req("g"), ctx + ".g"); m.curve_sigma_s = L.curve_ref(f.req("sigma_s"), ctx + ".sigma_s"); m.curve_sigma_a = L.curve_ref(f.req("sigma_a"), ctx + ".sigma_a");
        } else if (type == "Rayleigh") {
            m.kind = PT_MEDIUM_RAYLEIGH;
            m.curve_ior = L.curve_ref(f.req("ior"), ctx + ".ior"); m.corrective_factor = f.f32("corrective_factor");
        } else fail(ctx + ": unknown variant `" + type + "`");
        f.done();
        if (sf.mediums.size() >= 255) fail("more than 255 mediums");
        sf.mediums.push_back(m);
        sf.medium_ids[kv.first] = (int)sf.mediums.size();
    }

    // ---- scan: which materials and meshes the instances use (mod.rs:192-262)
    struct InstanceData { int kind = 0; std::string material; bool has_material = false; std::string mesh; bool has_index = false; bool has_transform = false; Mat4 fwd; pt_instance geo; };
    std::vector<InstanceData> idata;
    std::vector<std::string> used_materials, used_meshes;
    auto use = [](std::vector<std::string>& v, const std::string& s) { if (std::find(v.begin(), v.end(), s) == v.end()) v.push_back(s); };
    size_t inst_no = 0;
    for (auto& iv : *instances.a) {
        std::string ctx = "instances[" + std::to_string(inst_no++) + "]";
        Fields f(iv, ctx);
        InstanceData id; memset(&id.geo, 0, sizeof(id.geo));
        if (const toml::Value* mn = f.opt("material_name")) { if (mn->kind != toml::Value::String) fail(ctx + ".material_name: expected a string"); id.material = mn->s; id.has_material = true; use(used_materials, mn->s); }
        if (const toml::Value* tv = f.opt("transform")) {
            Fields tf(*tv, ctx + ".transform");
            float scale[3], translate[3];
            bool hs = tf.floats_opt("scale", scale, 3);
            std::vector<AxisAngle> rot;
            if (const toml::Value* rv = tf.opt("rotate")) rot = parse_rotations(*rv, ctx + ".transform.rotate");
            bool ht = tf.floats_opt("translate", translate, 3);
            tf.done();
            id.has_transform = true; id.fwd = from_stack(hs ? scale : nullptr, rot, ht ? translate : nullptr);
        }
        Fields af(f.req("aggregate"), ctx + ".aggregate");
        f.done();
        std::string type = af.str("type");
        if (type == "Rect") {
            id.kind = PT_SHAPE_RECT;
            af.floats("size", id.geo.size, 2); af.floats("origin", id.geo.origin, 3);
            id.geo.axis = enum_of(af.str("normal"), {"X", "Y", "Z"}, ctx + ".aggregate.normal");
            id.geo.two_sided = af.boolean("two_sided");
            if (!(id.geo.size[0] > 0.0f && id.geo.size[1] > 0.0f)) fail(ctx + ": rect size must be positive");  // primitives.rs:58
        } else if (type == "Sphere") {
            id.kind = PT_SHAPE_SPHERE; id.geo.radius = af.f32("radius"); af.floats("origin", id.geo.origin, 3);
            if (!(id.geo.radius > 0.0f)) fail(ctx + ": radius must be positive");
        } else if (type == "Disk") {
            id.kind = PT_SHAPE_DISK; id.geo.radius = af.f32("radius"); af.floats("origin", id.geo.origin, 3); id.geo.two_sided = af.boolean("two_sided");
            if (!(id.geo.radius > 0.0f)) fail(ctx + ": radius must be positive");
        } else if (type == "Mesh") {
            id.kind = PT_SHAPE_MESH; id.mesh = af.str("name"); id.has_index = af.has("index");
            if (id.has_index) af.integer("index", 0, 1 << 30);
            use(used_meshes, id.mesh);
        } else fail(ctx + ".aggregate: unknown variant `" + type + "`");
        // AggregateData has no deny_unknown_fields on the enum itself, but every variant struct has
        af.done();
        idata.push_back(id);
    }

    // ---- meshes: load the used ones, collect the materials their .mtl files name (mod.rs:215-262)
    struct LoadedMesh { std::string key; pth::ObjModel model; std::string prefix; };
    std::vector<LoadedMesh> loaded;
    std::map<std::string, std::vector<std::string>> mesh_materials;  // library name -> .mtl material names by index
    for (auto& kv : L.meshes_lib.table()->items) {
        if (std::find(used_meshes.begin(), used_meshes.end(), kv.first) == used_meshes.end()) continue;
        if (kv.first.find(';') != std::string::npos) fail("semicolon (;) disallowed in mesh names");
        Fields mf(kv.second, "meshes." + kv.first);
        std::string filename = mf.str("filename");
        int64_t mesh_index = mf.integer_or("mesh_index", 0, 1 << 30, -1);
        mf.done();
        pth::ObjFile obj; std::string err;
        if (!pth::load_obj(resolve_path(filename), &obj, &err)) fail(err);
        if (mesh_index >= 0) {
            if ((size_t)mesh_index >= obj.models.size()) fail("meshes." + kv.first + ": mesh_index out of range");
            loaded.push_back({kv.first, obj.models[(size_t)mesh_index], kv.first});
        } else {
            for (size_t k = 0; k < obj.models.size(); ++k) loaded.push_back({kv.first + ";" + std::to_string(k), obj.models[k], kv.first});
        }
        std::vector<std::string> names = obj.materials;
        for (auto& n : names) use(used_materials, n);
        if (names.empty()) names.push_back("error");
        mesh_materials[kv.first] = names;
    }
    for (auto& m : used_meshes) if (!mesh_materials.count(m)) fail("mesh `" + m + "` not found in the meshes library");

    // ---- environment first (its curves / texture), then materials in library order (mod.rs:264-437)
    {
        Fields ef(env, "environment");
        std::string type = ef.str("type");
        pt_environment& e = sf.desc.environment;
        memset(&e, 0, sizeof(e));
        e.curve = -1; e.texstack = -1; e.importance_luminance_curve = -1;
        store(identity(), e.rotation_forward); store(identity(), e.rotation_reverse);
        if (type == "Constant" || type == "Sun") {
            e.kind = type == "Constant" ? PT_ENV_CONSTANT : PT_ENV_SUN;
            bool ok = true;
            e.curve = L.curve_ref(ef.req("color"), "environment.color", &ok);
            if (!ok) { sf.warn("failed to resolve curve, falling back to error color"); e.curve = sf.curve_names["__mauve"]; }
            e.strength = ef.f32("strength");
            if (type == "Sun") {
                e.angular_diameter = ef.f32("angular_diameter");
                float d[3]; ef.floats("sun_direction", d, 3);
                float n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);  // Vec3::normalized, f32
                for (int k = 0; k < 3; ++k) e.sun_direction[k] = d[k] / n;
            }
        } else if (type == "HDRI") {
            e.kind = PT_ENV_HDR;
            std::string tex = ef.str("texture_name");
            e.strength = ef.f32("strength");
            if (const toml::Value* rv = ef.opt("rotation")) {
                Mat4 fwd = from_stack(nullptr, parse_rotations(*rv, "environment.rotation"), nullptr);
                store(fwd, e.rotation_forward); store(inverse(fwd), e.rotation_reverse);
            }
            e.texstack = L.texture_stack(tex);
            if (e.texstack < 0) {  // environment.rs:106-119: a 1x1 mauve texture
                sf.warn("importance map texture not found, using mauve texture");
                pt_texture_layer layer; memset(&layer, 0, sizeof(layer));
                layer.kind = PT_TEXTURE1; layer.curves[0] = sf.curve_names["__mauve"]; layer.curves[1] = layer.curves[2] = layer.curves[3] = -1;
                layer.width = layer.height = 1; layer.data_offset = sf.texture_data.size();
                sf.texture_data.push_back(1.0f);
                sf.layers.push_back(layer);
                pt_texstack ts; ts.first_layer = (int32_t)sf.layers.size() - 1; ts.layer_count = 1;
                sf.texstacks.push_back(ts);
                e.texstack = (int32_t)sf.texstacks.size() - 1;
            }
            if (const toml::Value* iv = ef.opt("importance_map")) {
                Fields mf(*iv, "environment.importance_map");
                int64_t w = mf.integer("width", 1, 1 << 20), h = mf.integer("height", 1, 1 << 20);
                bool cache = mf.boolean("cache");
                int lum = -1;
                if (const toml::Value* lv = mf.opt("luminance_curve")) lum = sf.add_curve(curve_from_data(*lv, "environment.importance_map.luminance_curve"));
                mf.done();
                // environment.rs:131-171: the map is baked only when cache is set and the strength is positive; otherwise it
                // stays ImportanceMap::Unbaked and the environment is sampled uniformly
                if (cache && e.strength > 0.0f) { e.importance_width = (int32_t)w; e.importance_height = (int32_t)h; e.importance_luminance_curve = lum; }
            }
        } else fail("environment: unknown variant `" + type + "`");
        ef.done();
    }
    for (auto& kv : L.materials_lib.table()->items) {
        if (std::find(used_materials.begin(), used_materials.end(), kv.first) == used_materials.end()) continue;
        L.material(kv.first, kv.second);
    }

    // ---- meshes -> flat arrays, with the .mtl names mapped to material ids (mod.rs:469-502)
    std::map<std::string, int> mesh_index_of;
    for (auto& lm : loaded) {
        const pth::ObjModel& m = lm.model;
        if (m.indices.empty()) fail("mesh " + lm.key + " has no faces");
        pt_mesh pm;
        pm.vertex_offset = (uint32_t)(sf.vertices.size() / 3); pm.vertex_count = (uint32_t)(m.positions.size() / 3);
        pm.index_offset = (uint32_t)sf.indices.size(); pm.face_count = (uint32_t)(m.indices.size() / 3);
        pm.normal_offset = -1;
        if (!m.normals.empty()) {
            if (m.normals.size() != m.positions.size()) fail("mesh " + lm.key + ": some vertices have normals and some do not");
            pm.normal_offset = (int32_t)(sf.normals.size() / 3);
            sf.normals.insert(sf.normals.end(), m.normals.begin(), m.normals.end());
        }
        sf.vertices.insert(sf.vertices.end(), m.positions.begin(), m.positions.end());
        sf.indices.insert(sf.indices.end(), m.indices.begin(), m.indices.end());
        const std::vector<std::string>& names = mesh_materials[lm.prefix];
        size_t mi = m.material >= 0 ? (size_t)m.material : 0;  // mesh.material_id.unwrap_or(0), meshes.rs:131
        uint32_t id = PT_MATERIAL_ID(PT_TAG_LIGHT, 0);
        if (mi < names.size() && sf.material_ids.count(names[mi])) id = sf.material_ids[names[mi]];
        else sf.warn("setting material ids to 0 since " + (mi < names.size() ? names[mi] : std::string("<none>")) + " was not found in the materials library");
        pm.face_material_offset = (int32_t)sf.face_materials.size();
        sf.face_materials.insert(sf.face_materials.end(), pm.face_count, id);
        mesh_index_of[lm.key] = (int)sf.meshes.size();
        sf.meshes.push_back(pm);
    }

    // ---- instances (mod.rs:504-551, instance.rs:73-118)
    auto material_of = [&](const InstanceData& id, size_t n) -> uint32_t {
        if (!id.has_material) return PT_MATERIAL_NONE;
        auto it = sf.material_ids.find(id.material);
        if (it != sf.material_ids.end()) return it->second;
        sf.warn("material not found in mapping, instance " + std::to_string(n) + ", material name " + id.material);
        return sf.material_ids["error"];
    };
    for (auto& id : idata) {
        pt_instance inst = id.geo;
        inst.kind = id.kind; inst.has_transform = id.has_transform ? 1 : 0; inst.mesh = -1;
        Mat4 fwd = id.has_transform ? id.fwd : identity();
        store(fwd, inst.forward); store(id.has_transform ? inverse(fwd) : identity(), inst.reverse);
        if (id.kind == PT_SHAPE_MESH && !id.has_index) {
            // mesh bundle (mod.rs:507-535): one instance per loaded mesh whose key starts with the name (key order here;
            // the reference iterates a HashMap)
            bool any = false;
            for (auto& kv : mesh_index_of) {
                if (kv.first.compare(0, id.mesh.size(), id.mesh) != 0) continue;
                inst.mesh = kv.second; inst.material = material_of(id, sf.instances.size());
                sf.instances.push_back(inst); any = true;
            }
            if (!any) fail("mesh map did not contain mesh " + id.mesh);
        } else {
            if (id.kind == PT_SHAPE_MESH) {
                auto it = mesh_index_of.find(id.mesh);  // parse_with looks the plain name up (primitives.rs:72-75)
                if (it == mesh_index_of.end()) fail("mesh map did not contain mesh " + id.mesh + " (an instance with `index` needs a library entry with `mesh_index`)");
                inst.mesh = it->second;
            }
            inst.material = material_of(id, sf.instances.size());
            sf.instances.push_back(inst);
        }
    }

    // ---- cameras (cameras.rs:116-204): one per render-settings entry when a config is given
    std::map<std::string, pt_camera> by_name;
    std::vector<std::string> file_order;
    size_t cam_no = 0;
    for (auto& cv : *cameras.a) {
        std::string ctx = "cameras[" + std::to_string(cam_no++) + "]";
        Fields f(cv, ctx);
        std::string type = f.str("type"), name = f.str("name");
        pt_camera c; memset(&c, 0, sizeof(c));
        if (type == "PanoramaCamera") {  // PanoramaCameraData, cameras.rs:86-94,150-159
            c.kind = PT_CAMERA_PANORAMA;
            f.floats("look_from", c.look_from, 3); f.floats("look_at", c.look_at, 3);
            float up[3] = {0.0f, 0.0f, 1.0f};
            f.floats_opt("v_up", up, 3);
            float n = std::sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
            for (int k = 0; k < 3; ++k) c.v_up[k] = up[k] / n;
            f.floats("fov", c.fov, 2);
            f.done();
            by_name[name] = c; file_order.push_back(name);
            continue;
        }
        if (type != "SimpleCamera") {
            if (type != "RealisticCamera") fail(ctx + ": unknown variant `" + type + "`");
            bool used = false;
            if (config) for (auto& s : config->settings) used = used || s->camera_id == name;
            if (used) fail(ctx + ": camera type `" + type + "` is not on the PT path", PT_ERR_UNSUPPORTED);
            sf.warn(ctx + ": camera type `" + type + "` is not on the PT path, skipped");
            continue;
        }
        f.floats("look_from", c.look_from, 3); f.floats("look_at", c.look_at, 3);
        float up[3] = {0.0f, 0.0f, 1.0f};
        f.floats_opt("v_up", up, 3);
        float n = std::sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
        for (int k = 0; k < 3; ++k) c.v_up[k] = up[k] / n;
        c.vfov = f.f32("vfov"); c.focal_distance = f.f32_or("focal_distance", 10.0f); c.aperture_diameter = f.f32_or("aperture_diameter", 0.01f);
        f.f32_or("lens_diameter", 0.01f);
        if (const toml::Value* av = f.opt("aperture")) {
            Fields af(*av, ctx + ".aperture");
            std::string at = af.str("type");
            if (at == "Bladed") { af.integer("blades", 0, 255); af.f32("sharpness"); sf.warn(ctx + ": bladed apertures are sampled as circular on this path"); }
            else if (at != "Circular") fail(ctx + ".aperture: unknown variant `" + at + "`");
            af.done();
        }
        f.done();
        by_name[name] = c; file_order.push_back(name);
    }
    if (config) {
        for (auto& s : config->settings) {
            auto it = by_name.find(s->camera_id);
            if (it == by_name.end()) fail("camera `" + s->camera_id + "` named by the render settings is not in the scene");
            if (!sf.camera_names.count(s->camera_id)) sf.camera_names[s->camera_id] = (int)sf.cameras.size();  // camera_names_to_index
            sf.cameras.push_back(it->second);
        }
    } else {
        for (auto& n : file_order) { sf.camera_names[n] = (int)sf.cameras.size(); sf.cameras.push_back(by_name[n]); }
    }
    if (sf.cameras.empty()) fail("the scene has no usable camera");
    build_desc(sf);
}

void load_config(const std::string& path, pt_config& cfg) {
    toml::Value root = parse_file(path);
    Fields top(root, path);
    if (top.has("env_sampling_probability")) { cfg.has_env_prob = true; cfg.env_prob = top.f32("env_sampling_probability"); }
    cfg.scene_file = top.str("default_scene_file");
    {
        Fields rf(top.req("renderer"), "renderer");
        std::string type = rf.str("type");
        if (type == "Naive") cfg.renderer = PT_RENDERER_NAIVE;
        else if (type == "Tiled") {
            cfg.renderer = PT_RENDERER_TILED;
            const toml::Value& ts = rf.req("tile_size");
            if (ts.kind != toml::Value::ArrayKind || ts.a->size() != 2 || (*ts.a)[0].kind != toml::Value::Integer || (*ts.a)[1].kind != toml::Value::Integer) fail("renderer.tile_size: expected [width, height]");
            cfg.tile_w = (uint32_t)(*ts.a)[0].i; cfg.tile_h = (uint32_t)(*ts.a)[1].i;
            if (cfg.tile_w == 0 || cfg.tile_h == 0 || cfg.tile_w > 65535 || cfg.tile_h > 65535) fail("renderer.tile_size out of range");
        } else if (type == "Preview") fail("renderer type Preview is not supported", PT_ERR_UNSUPPORTED);
        else fail("renderer: unknown variant `" + type + "`");
        rf.done();
    }
    const toml::Value& rs = top.req("render_settings");
    top.done();
    if (rs.kind != toml::Value::ArrayKind) fail("render_settings: expected an array of tables");
    size_t n = 0;
    for (auto& sv : *rs.a) {
        std::string ctx = "render_settings[" + std::to_string(n++) + "]";
        Fields f(sv, ctx);
        auto st = std::make_unique<pt_config::Settings>();
        pt_render_settings& s = st->s;
        memset(&s, 0, sizeof(s));
        if (const toml::Value* fv = f.opt("filename")) { if (fv->kind != toml::Value::String) fail(ctx + ".filename: expected a string"); st->filename = fv->s; st->has_filename = true; }
        { Fields r(f.req("resolution"), ctx + ".resolution"); s.width = (uint32_t)r.integer("width", 1, 1 << 16); s.height = (uint32_t)r.integer("height", 1, 1 << 16); r.done(); }
        {
            Fields i(f.req("integrator"), ctx + ".integrator");
            std::string type = i.str("type");
            if (type == "PT") { s.integrator = PT_INTEGRATOR_PT; s.light_samples = (uint32_t)i.integer("light_samples", 0, 65535); s.medium_aware = i.boolean("medium_aware"); }
            else if (type == "LT") { s.integrator = PT_INTEGRATOR_LT; s.camera_samples = (uint32_t)i.integer("camera_samples", 0, 65535); }
            else fail(ctx + ".integrator: unknown variant `" + type + "`");
            i.done();
        }
        s.min_bounces = (int32_t)f.integer_or("min_bounces", 0, 65535, -1);
        s.max_bounces = (int32_t)f.integer_or("max_bounces", 0, 65535, -1);
        s.hwss = f.boolean("hwss");
        s.threads = (int32_t)f.integer_or("threads", 0, 65535, -1);
        s.min_samples = (uint32_t)f.integer("min_samples", 0, 65535);
        if (f.has("exposure")) f.f32("exposure");  // TOMLRenderSettings::exposure is accepted and dropped (config.rs:76,92-111)
        s.max_samples = (int32_t)f.integer_or("max_samples", 0, 65535, -1);
        st->camera_id = f.str("camera_id");
        s.russian_roulette = f.tri_bool("russian_roulette");
        s.only_direct = f.tri_bool("only_direct");
        float wb[2];
        if (f.floats_opt("wavelength_bounds", wb, 2)) { s.has_wavelength_bounds = 1; s.wavelength_lo = wb[0]; s.wavelength_hi = wb[1]; }
        if (f.has("premultiply")) { s.has_premultiply = 1; s.premultiply = f.f32("premultiply"); } else s.premultiply = 1.0f;
        { Fields c(f.req("colorspace_settings"), ctx + ".colorspace_settings"); s.colorspace = enum_of(c.str("type"), {"sRGB", "Rec709", "Rec2020"}, ctx + ".colorspace_settings"); c.done(); }
        {
            Fields t(f.req("tonemap_settings"), ctx + ".tonemap_settings");
            s.tonemap = enum_of(t.str("type"), {"Clamp", "Reinhard0", "Reinhard1"}, ctx + ".tonemap_settings");
            s.key_value = 0.18f; s.white_point = 1.0f;
            if (s.tonemap == PT_TONEMAP_CLAMP) { if (t.has("exposure")) { s.has_exposure = 1; s.exposure = t.f32("exposure"); } }
            else { s.key_value = t.f32("key_value"); if (s.tonemap == PT_TONEMAP_REINHARD1) s.white_point = t.f32("white_point"); }
            s.luminance_only = t.boolean("luminance_only");
            if (const toml::Value* sv2 = t.opt("silenced")) { if (sv2->kind != toml::Value::Boolean) fail(ctx + ".tonemap_settings.silenced: expected a boolean"); s.silenced = sv2->b; }
            t.done();
        }
        f.done();
        cfg.settings.push_back(std::move(st));
    }
    for (auto& st : cfg.settings) { st->s.filename = st->has_filename ? st->filename.c_str() : nullptr; st->s.camera_id = st->camera_id.c_str(); }
}

template <typename F>
pt_status guarded(F&& body) {
    try { body(); return PT_OK; }
    catch (const Failure& f) { g_error = f.message; return f.status; }
    catch (const std::exception& e) { g_error = e.what(); return PT_ERR_INVALID_ARGUMENT; }
}

}  // namespace

extern "C" {

const char* pt_scene_file_last_error(void) { return g_error.c_str(); }
void pt_scene_file_set_root(const char* directory) { g_root = directory ? directory : ""; }

pt_status pt_config_load(const char* path, pt_config** out) {
    if (!path || !out) { g_error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    auto cfg = std::make_unique<pt_config>();
    pt_status st = guarded([&] { load_config(path, *cfg); });
    if (st == PT_OK) *out = cfg.release();
    return st;
}
void pt_config_free(pt_config* c) { delete c; }
const char* pt_config_scene_file(const pt_config* c) { return c ? c->scene_file.c_str() : nullptr; }
int32_t pt_config_renderer(const pt_config* c, uint32_t* tw, uint32_t* th) {
    if (!c) return -1;
    if (tw) *tw = c->tile_w;
    if (th) *th = c->tile_h;
    return c->renderer;
}
uint32_t pt_config_render_settings_count(const pt_config* c) { return c ? (uint32_t)c->settings.size() : 0; }
pt_status pt_config_render_settings(const pt_config* c, uint32_t i, pt_render_settings* out) {
    if (!c || !out || i >= c->settings.size()) { g_error = "render settings index out of range"; return PT_ERR_INVALID_ARGUMENT; }
    *out = c->settings[i]->s;
    return PT_OK;
}
pt_status pt_config_render_desc(const pt_config* c, uint32_t i, uint64_t seed, pt_render_desc* out) {
    if (!c || !out || i >= c->settings.size()) { g_error = "render settings index out of range"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_render_settings& s = c->settings[i]->s;
    if (s.integrator != PT_INTEGRATOR_PT) { g_error = "only the PT integrator is on this path"; return PT_ERR_UNSUPPORTED; }

    if (s.max_bounces < 0) { g_error = "max_bounces is required (the reference unwrap()s it, src/integrator/mod.rs:97)"; return PT_ERR_INVALID_ARGUMENT; }
    memset(out, 0, sizeof(*out));
    out->width = s.width; out->height = s.height; out->spp = s.min_samples;
    out->min_bounces = s.min_bounces >= 0 ? (uint32_t)s.min_bounces : 4u;
    out->max_bounces = (uint32_t)s.max_bounces;
    out->light_samples = s.light_samples;
    out->only_direct = s.only_direct == 1;
    out->wavelength_lo = s.has_wavelength_bounds ? s.wavelength_lo : 380.0f;
    out->wavelength_hi = s.has_wavelength_bounds ? s.wavelength_hi : 750.0f;
    out->camera_index = 0;  // the PT integrator always asks for camera 0 (src/renderer/tiled.rs:378)
    out->seed = seed;
    if (c->renderer == PT_RENDERER_TILED) { out->tile_width = c->tile_w; out->tile_height = c->tile_h; }
    else {  // NaiveRenderer (src/renderer/naive.rs:67-103): pixels in row-major order, all samples summed, one division
        out->tile_width = s.width; out->tile_height = s.height; out->phase_samples = s.min_samples;
    }
    out->medium_aware = s.medium_aware ? 1u : 0u;   // random_walk_medium (src/integrator/pt.rs:447)
    // `hwss` is parsed by the reference (src/parsing/config.rs:51) and read by nothing on the PT path: a no-op here too.  The engine's
    // hero-wavelength variant is asked for explicitly (pt_render_desc.hero_wavelengths; ptcli --hero-wavelengths 4).
    out->hero_wavelengths = 1u;
    return PT_OK;
}
pt_status pt_config_output_desc(const pt_config* c, uint32_t i, float factor, pt_output_desc* out) {
    if (!c || !out || i >= c->settings.size()) { g_error = "render settings index out of range"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_render_settings& s = c->settings[i]->s;
    memset(out, 0, sizeof(*out));
    out->width = s.width; out->height = s.height; out->tonemap = s.tonemap; out->luminance_only = s.luminance_only;
    out->exposure = s.has_exposure ? s.exposure : 0.0f; out->key_value = s.key_value; out->white_point = s.white_point;
    out->colorspace = s.colorspace; out->factor = factor * s.premultiply;
    return PT_OK;
}

pt_status pt_scene_file_load(const char* scene_path, const pt_config* config, pt_scene_file** out) {
    if (!scene_path || !out) { g_error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    auto sf = std::make_unique<pt_scene_file>();
    pt_status st = guarded([&] { load_scene(scene_path, config, *sf); });
    if (st == PT_OK) *out = sf.release();
    return st;
}
void pt_scene_file_free(pt_scene_file* s) { delete s; }
const pt_scene_desc* pt_scene_file_desc(const pt_scene_file* s) { return s ? &s->desc : nullptr; }
int64_t pt_scene_file_material(const pt_scene_file* s, const char* name) { auto it = s->material_ids.find(name); return it == s->material_ids.end() ? -1 : (int64_t)it->second; }
const char* pt_scene_file_material_name(const pt_scene_file* s, uint32_t material_id) {
    if (!s) return nullptr;
    const char* found = nullptr;   // ("error" shares light 0's id with the first light material: the library's own name wins where there is one)
    for (const auto& kv : s->material_ids)
        if (kv.second == material_id && (!found || kv.first != "error")) found = kv.first.c_str();
    return found;
}
int32_t pt_scene_file_curve(const pt_scene_file* s, const char* name) { auto it = s->curve_names.find(name); return it == s->curve_names.end() ? -1 : it->second; }
int32_t pt_scene_file_texture(const pt_scene_file* s, const char* name) { auto it = s->texture_names.find(name); return it == s->texture_names.end() ? -1 : it->second; }
int32_t pt_scene_file_camera(const pt_scene_file* s, const char* name) { auto it = s->camera_names.find(name); return it == s->camera_names.end() ? -1 : it->second; }
pt_status pt_scene_file_library_curve(pt_scene_file* s, const char* name, pt_curve* curve, const float** data, uint32_t* data_floats) {
    if (!s || !name || !curve || !data || !data_floats) { g_error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    return guarded([&] {
        auto it = s->library_curves.find(name);
        if (it == s->library_curves.end()) {
            const toml::Value* v = s->curves_library.table() ? s->curves_library.table()->find(name) : nullptr;
            if (!v) fail(std::string("curve `") + name + "` not found in the curves library");
            it = s->library_curves.emplace(name, curve_from_data(*v, std::string("curves.") + name)).first;
        }
        const CurveM& c = it->second;
        curve->kind = c.kind; curve->mode = c.mode; curve->p0 = c.p0; curve->p1 = c.p1; curve->data_offset = 0; curve->data_count = c.count;
        *data = c.data.data(); *data_floats = (uint32_t)c.data.size();
    });
}
uint32_t pt_scene_file_warning_count(const pt_scene_file* s) { return s ? (uint32_t)s->warnings.size() : 0; }
const char* pt_scene_file_warning(const pt_scene_file* s, uint32_t i) { return (s && i < s->warnings.size()) ? s->warnings[i].c_str() : nullptr; }

pt_status pt_image_read(const char* path, int32_t kind, float alpha_fill, uint32_t* width, uint32_t* height, uint32_t* channels, float** data) {
    if (!path || !width || !height || !channels || !data) { g_error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    pth::Image img; std::string err;
    const std::string p = resolve_path(path);
    bool ok = kind == PT_IMAGE_GREY8 ? pth::read_grey8(p, &img, &err) : kind == PT_IMAGE_RGBA8 ? pth::read_rgba8(p, &img, &err)
            : kind == PT_IMAGE_HDR ? pth::read_hdr(p, alpha_fill, &img, &err) : kind == PT_IMAGE_EXR ? pth::read_exr(p, &img, &err) : false;
    if (!ok) { g_error = err.empty() ? "unknown image kind" : err; return PT_ERR_INVALID_ARGUMENT; }
    float* out = (float*)malloc(sizeof(float) * (img.data.size() ? img.data.size() : 1));
    if (!out) { g_error = "out of memory"; return PT_ERR_OUT_OF_MEMORY; }
    memcpy(out, img.data.data(), sizeof(float) * img.data.size());
    *width = img.width; *height = img.height; *channels = img.channels; *data = out;
    return PT_OK;
}
void pt_image_free(float* data) { free(data); }

}  // extern "C"
