#include "pt_plan.h"
#include "pt_denoise_rules.h"
#include "pt_guides_chain_rules.h"
#include "pt_matte_rules.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pth {

std::vector<uint32_t> shard_pixels(uint32_t width, uint32_t height, uint32_t tw, uint32_t th, uint32_t shard_index, uint32_t shard_count) {
    struct T { uint32_t x0, x1, y0, y1; };
    std::vector<T> tiles;
    uint32_t fx = width / tw, fy = height / th, rx = width % tw, ry = height % th;
    for (uint32_t y = 0; y < fy; ++y) for (uint32_t x = 0; x < fx; ++x) tiles.push_back(T{x * tw, x * tw + tw, y * th, y * th + th});
    if (rx) for (uint32_t y = 0; y < fy; ++y) tiles.push_back(T{fx * tw, fx * tw + rx, y * th, y * th + th});
    if (ry) {
        for (uint32_t x = 0; x < fx; ++x) tiles.push_back(T{x * tw, x * tw + tw, fy * th, fy * th + ry});
        if (rx) tiles.push_back(T{fx * tw, fx * tw + rx, fy * th, fy * th + ry});
    }
    std::vector<uint32_t> mine;
    for (size_t t = 0; t < tiles.size(); ++t)
        if (!shard_count || PT_TILE_SHARD((uint32_t)t, fx, shard_count) == shard_index) mine.push_back((uint32_t)t);
    // The order of the tiles in the slot space is free (a pixel's samples are keyed by its id, its sums are its own), and it decides
    // how evenly the work falls on the workgroups, each of which takes a run of consecutive slots = a few consecutive tiles: in film
    // order those are neighbours and cost alike (a run of bright floor, a run of dark wall); taken with a stride coprime to their
    // number (about 0.382 of it), every run mixes tiles from all over the film.
    const size_t n = mine.size();
    size_t stride = (size_t)((double)n * 0.3819660112501051);
    auto gcd = [](size_t a, size_t b) { while (b) { size_t t = a % b; a = b; b = t; } return a; };
    if (stride < 1) stride = 1;
    while (gcd(stride, n ? n : 1) != 1) ++stride;
    std::vector<uint32_t> px;
    for (size_t i = 0; i < n; ++i) {
        const T& tile = tiles[mine[(i * stride) % n]];
        for (uint32_t y = tile.y0; y < tile.y1; ++y)
            for (uint32_t x = tile.x0; x < tile.x1; ++x) px.push_back(y * width + x);
    }
    return px;
}

PassSchedule schedule_passes(uint32_t n_passes, uint32_t bounces, int32_t skew_bounce, bool overlap) {
    PassSchedule sch;
    sch.steps.assign(n_passes, PassStep{0u, false, -1, -1, -1});
    if (!overlap || n_passes < 2) return sch;
    const int32_t g = (skew_bounce < 0 || bounces == 0) ? -1 : (skew_bounce < (int32_t)bounces ? skew_bounce : (int32_t)bounces - 1);
    for (uint32_t p = 0; p < n_passes; ++p) {
        PassStep& s = sch.steps[p];
        s.lane = p & 1u;
        s.wait_fork = p == 1;
        s.start_after = (p > 0 && g >= 0) ? (int32_t)p - 1 : -1;
        s.accumulate_after = p > 0 ? (int32_t)p - 1 : -1;
        s.signal_bounce = p + 1 < n_passes ? g : -1;
    }
    // (an even last pass has waited for the odd one before it in its accumulate stage: the caller's stream is already behind everything)
    sch.join_pass = ((n_passes - 1) & 1u) ? (int32_t)n_passes - 1 : -1;
    return sch;
}

std::vector<Pass> plan_passes(uint32_t n_pixels, uint32_t first_sample, uint32_t sample_count, uint32_t capacity, uint32_t phase_samples) {
    std::vector<Pass> passes;
    if (n_pixels == 0 || sample_count == 0) return passes;
    // A pass must be able to hold one whole phase (10 samples — or all of them for the naive renderer —, or the whole range
    // if shorter) of its pixels, because the per-phase partial sums of tiled.rs:366-391 live in registers of the
    // accumulate kernel.
    const uint32_t period = phase_samples ? phase_samples : 10;
    uint32_t phase = sample_count < period ? sample_count : period;
    uint32_t max_chunk = capacity / phase;
    if (max_chunk == 0) max_chunk = 1;
    uint32_t n_chunks = (n_pixels + max_chunk - 1) / max_chunk;
    uint32_t chunk = (n_pixels + n_chunks - 1) / n_chunks;   // even split
    for (uint32_t p0 = 0; p0 < n_pixels; p0 += chunk) {
        uint32_t pc = (n_pixels - p0 < chunk) ? n_pixels - p0 : chunk;
        uint32_t max_s = capacity / pc;
        if (max_s < phase) max_s = phase;                     // only when capacity < phase (degenerate)
        uint32_t s = first_sample, end = first_sample + sample_count;
        while (s < end) {
            uint32_t take = end - s; if (take > max_s) take = max_s;
            uint32_t stop = s + take;
            if (stop < end) {                                 // end the pass on a phase boundary
                uint32_t aligned = (stop / period) * period;
                if (aligned > s) stop = aligned;
            }
            passes.push_back(Pass{p0, pc, s, stop - s});
            s = stop;
        }
    }
    return passes;
}

// the value a tuning field stands for (0 = "the default" in the struct)
static uint32_t tuned(uint32_t value, uint32_t dflt) { return value ? value : dflt; }

// whether any instance of the flattened scene is a mesh (a scene without one never parks at a mesh: its top-level walks are the ones worth leaving early)
static bool scene_has_mesh(const std::vector<uint32_t>& blob) {
    const uint32_t off = blob[PT_HDR_INSTANCE_OFF], n = blob[PT_HDR_INSTANCE_COUNT];
    for (uint32_t i = 0; i < n; ++i) if (blob[off + i * PT_INST_WORDS + PT_INST_KIND] == (uint32_t)PT_SHAPE_MESH) return true;
    return false;
}

ScenePlan plan_scene(const pt_tuning& tn, std::vector<uint32_t>& blob) {
    using namespace ptk;
    ScenePlan sp;
    uint32_t& flags = blob[PT_HDR_FLAGS];
    const uint32_t switches[][2] = {{PT_TUNE_EXACT_SLAB, PT_FLAG_EXACT_SLAB}, {PT_TUNE_NO_CULL, PT_FLAG_NO_CULL}, {PT_TUNE_NO_SWEEP, PT_FLAG_NO_SWEEP},
                                    {PT_TUNE_NO_MESH_SWEEP, PT_FLAG_NO_MESH_SWEEP}, {PT_TUNE_NO_KNOWN_LIGHT, PT_FLAG_NO_KNOWN_LIGHT}, {PT_TUNE_NO_ONE_LIGHT, PT_FLAG_NO_ONE_LIGHT}};
    for (const auto& s : switches) if (tn.flags & s[0]) flags |= s[1];
    if (tn.flags & PT_TUNE_NO_CONVEX) flags &= ~PT_FLAG_CONVEX;   // (the vertex code looks at an instance's certificate only under this flag, and only it makes marks)
    if (blob[PT_HDR_LIGHT_COUNT] > tuned(tn.light_prepass_max, kLightPrepassMax)) flags |= PT_FLAG_NO_LIGHT_PREPASS;
    bool any_xf = false;
    for (uint32_t i = 0; i < blob[PT_HDR_INSTANCE_COUNT]; ++i) {
        const uint32_t inst = blob[PT_HDR_INSTANCE_OFF] + i * PT_INST_WORDS;
        any_xf = any_xf || (blob[inst + PT_INST_FLAGS] & 1u) != 0u;
        // (the mesh records' inner ball and slab table: mesh_surely_blocks / mesh_surely_missed claim nothing without them)
        if ((tn.flags & PT_TUNE_NO_MESH_SHORTCUTS) && blob[inst + PT_INST_KIND] == (uint32_t)PT_SHAPE_MESH) { blob[blob[inst + PT_INST_MESH] + PT_MESH_INNER_R] = 0u; blob[blob[inst + PT_INST_MESH] + PT_MESH_DOP_OFF] = 0u; }
    }
    // no instance carries a transform (the Cornell box): the forms without the matrix paths (PT_AMD_GENERAL_FORMS=1 keeps the general ones)
    // "no lights" = no hit can carry a Light tag: the light list is empty AND no mesh instance overrides its material with a light
    // (such a mesh is not in the light list, world/mod.rs:45-54, but its hits emit and take no light samples: PT_FLAG_NO_SHADOW_BOUND)
    const bool no_light_hits = blob[PT_HDR_LIGHT_COUNT] == 0u && !(flags & PT_FLAG_NO_SHADOW_BOUND);
    sp.lacks = (tn.flags & PT_TUNE_GENERAL_FORMS) ? 0u : ((any_xf ? 0u : PT_SCENE_NO_XF) | (no_light_hits ? PT_SCENE_NO_LIGHTS : 0u));
    const uint32_t all_limit = std::min(tuned(tn.lds_all_limit, kLdsAllLimitBytes), kLdsBlobLimitBytes);   // (experiments: the largest blob staged whole)
    sp.lds_mode = (tn.flags & PT_TUNE_NO_LDS) ? PT_LDS_NONE : (uint32_t)blob.size() * 4 <= all_limit ? PT_LDS_ALL
                : (blob[PT_HDR_CORE_WORDS] * 4 <= kLdsBlobLimitBytes && !(tn.flags & PT_TUNE_NO_CORE_LDS)) ? PT_LDS_CORE : PT_LDS_NONE;
    return sp;
}

bool plan_render(const std::vector<uint32_t>& blob, const pt_tuning& tn, const ScenePlan& scene, const RenderAsk& ask, RenderPlan* plan, std::string* error) {
    using namespace ptk;
    using namespace ptd;
    const pt_render_desc& rd = ask.rd;
    const pt_adaptive_desc* adaptive = ask.adaptive;
    const uint32_t blob_bytes = (uint32_t)blob.size() * 4u, flags = blob[PT_HDR_FLAGS];
    const int mode = scene.lds_mode;
    RenderPlan& p = *plan;
    p = RenderPlan();

    // ---- the queues: capacity, grid, layouts
    p.capacity = tuned(tn.batch_slots, 1u << 27);  // path slots per pass (128 Mi ~ 32 GB of queues of the 288 GB; tools/sweep.sh)
    if (p.capacity < 1024) p.capacity = 1024;
    const uint64_t want = (uint64_t)ask.n_pixels * (adaptive ? std::max(adaptive->step, rd.spp) : rd.sample_count);   // (the longest pass of a round)
    if (want < p.capacity) p.capacity = (uint32_t)(want ? want : 1);
    const uint32_t blocks_per_cu = tuned(tn.blocks_per_cu, 64);
    if (blocks_per_cu > 1024) { *error = "pt_tuning::blocks_per_cu (PT_AMD_BLOCKS_PER_CU) must be in 1..1024"; return false; }
    p.grid = ask.num_cus * (int)blocks_per_cu;  // queue segments = workgroups per launch
    // a pass holds at least one whole phase of one pixel (plan_passes): the queues must too (NaiveRenderer settings: phase = spp)
    p.capacity = std::max(p.capacity, std::min(rd.sample_count, rd.phase_samples));
    p.hero = rd.hero_wavelengths == 4;
    if (p.hero && p.capacity > (1u << 26)) p.capacity = 1u << 26;  // 4-wavelength queues are ~1.5x wider: 64 Mi slots ~ 24 GB
    // (a queue's tiles are laid out by the number of fields this render uses, pt_stages.h: the buffers are sized for the widest layout seen)
    // (the medium-aware walk keeps its two extra path fields where the hero layout keeps the passengers' throughputs)
    const uint32_t item_samples = rd.light_samples ? rd.light_samples : 1;
    p.path_fields = p.hero ? Layout<4>::path_fields : (rd.medium_aware ? (uint32_t)PS_FIELDS + 2u : Layout<1>::path_fields);
    p.item_fields = p.hero ? Layout<4>::shadow_queue_fields(item_samples) : Layout<1>::shadow_queue_fields(item_samples);
    p.lds_bytes = mode == PT_LDS_ALL ? blob_bytes : (mode == PT_LDS_CORE ? blob[PT_HDR_CORE_WORDS] * 4u : 0u);

    // ---- the traversal form
    const bool sweep = blob[PT_HDR_SWEEP_OFF] != 0 && !(flags & PT_FLAG_NO_SWEEP);
    // the sweep table holds walked meshes: rays that reach one are parked and resumed in full waves (PT_AMD_NO_PARK=1: in line)
    const bool walks = (flags & PT_FLAG_SWEEP_WALKS) != 0;
    p.mesh_lights = blob[PT_HDR_LIGHT_FACE_OFF] != 0u;   // (emissive mesh faces: PT_FORM_ANY, below)
    const bool routed = ask.routed;   // (a light-group, path-pass or path-expression render: PT_FORM_ANY and the FULL vertex form, whose siblings route the energy: pt_kern_routed.hip)
    // (the parked forms run where ensure_buffers makes the parked kernels' scratch, b.park — a table with walked meshes, or no table: the two cases below)
    const bool may_park = !(tn.flags & PT_TUNE_NO_PARK) && !p.mesh_lights && !routed;
    const bool parked = sweep && walks && may_park;
    // no sweep table (more than 64 instances, PT_AMD_NO_SWEEP): the top-level tree per lane, every mesh parked (top_walk_run, pt_device.h)
    const bool parked_walk = !sweep && may_park;
    // PT_AMD_POOL=1: phase 3 of a pure sweep scene pooled per wave (sweep_run_pooled).  Bit-identical, but measured slower than the lane
    // loop on MI355X (C2: k_extend 3155 vs 2475 us, k_shadow 5421 vs 4677 us; DESIGN.md section 5 has the breakdown), so it is not the default.
    // (the pooled kernels are not in the product: make EXTRA=-DPT_EXPERIMENTS builds them, PT_AMD_POOL=1 selects them there)
    const bool pooled = ask.pool_lds_bytes != 0u && sweep && !walks && mode == PT_LDS_ALL && p.lds_bytes + ask.pool_lds_bytes <= kLdsBlobLimitBytes && (tn.flags & PT_TUNE_EXPERIMENT_POOL) != 0;
    // (walked meshes in line under PT_AMD_NO_PARK, and every partly staged or unstaged blob: the run-time choice of PT_FORM_ANY.  A scene with emissive mesh faces
    // takes it too: the specialised traversal forms are compiled without the faces' code — PT_SCENE_NO_MESH_LIGHTS, pt_kern_*.hip — and keep their registers)
    p.trav_form = parked ? PT_FORM_PARKED : parked_walk ? PT_FORM_PARKED_WALK : (mode != PT_LDS_ALL || (sweep && walks) || p.mesh_lights || routed) ? PT_FORM_ANY
                : pooled ? PT_FORM_POOLED : sweep ? PT_FORM_SWEEP : PT_FORM_WALK;

    // ---- the parked kernels' variants
    // the parked kernels in workgroups of 512 / 1024 threads that stage the whole blob (pt_tuning::park_block): static form, one wavelength, a blob that fits
    // 0 = the measured default: the light-sample kernel in workgroups of 512 (C3: -5 %), the closest-hit kernel in its own 256 (at 512 it loses its fifth wave
    // per SIMD: +14 %); 512 / 1024 = both kernels; 256 = neither (profiles/r4_experiments.md section 1)
    const bool park_big_ok = !p.hero && blob_bytes <= kParkBlobLimitBytes && mode == PT_LDS_CORE && !(tn.flags & PT_TUNE_NO_LDS);
    // (round 6: in a scene with a certified convex body — PT_FLAG_CONVEX, the gem of C3 — nine in ten of the light rays that used to walk the mesh no longer reach it, and the
    // light-sample kernel is better off in workgroups of 256 that stage the core alone, twice the workgroups per CU: C3 k_shadow_parked 2339 -> 2083 us, profiles/r6d_ab_park.txt)
    const bool few_walks = (flags & PT_FLAG_CONVEX) != 0u;
    p.park_block = !park_big_ok ? (uint32_t)kBlock : tn.park_block == 0u ? (few_walks ? (uint32_t)kBlock : 512u) : tn.park_block;
    p.park_block_extend = !park_big_ok || tn.park_block == 0u ? (uint32_t)kBlock : tn.park_block;
    // The parked kernels take units of work from a counter, a few persistent workgroups per CU, when the whole blob is staged in LDS
    // (C3: k_extend 9175 -> 7880 us, k_shadow 8008 -> 7105, 487 -> 543 Msamples/s: park lists that live across units keep the drains
    // full).  With the mesh in HBM/L2 (C4) the static form wins, 1128 vs 1083 Msamples/s: a wave's parked rays then come from one
    // region of the film and walk the same part of the mesh.  PT_AMD_PARK_DYNAMIC=0 / 1 forces either.
    p.park_dynamic = parked && (tn.park_dynamic < 0 ? mode == PT_LDS_ALL : tn.park_dynamic != 0);
    p.park_big = parked && !p.park_dynamic && p.park_block != (uint32_t)kBlock && mode != PT_LDS_ALL;
    p.dyn_grid = std::min(ask.num_cus * (int)tuned(tn.park_blocks_per_cu, 4), p.grid);
    if (p.park_big) { p.launch_park_block = (int)p.park_block; p.launch_park_block_extend = (int)p.park_block_extend; p.park_blob_bytes = blob_bytes; }

    // ---- the walk-policy word
    // The top-level walk is left early by a wave's last lanes (top_walk_run) where that walk is long and nothing else thins the wave out: a tree of more than 64
    // instances — the scenes that have no sweep table by themselves — without a mesh (test_bokeh.toml + a floor: k_shadow_parked 2900 -> 2320 us at 32, 2430 at 16 and
    // at 48).  With a mesh in the scene the lanes of a wave PARK at it, the wave thins out although its rays are not done, and evicting the rest only adds park
    // traffic: the same scene with the gem standing on the floor 1337 -> 1260 Msamples/s at 32 (1341 at 16); a small scene forced off its table (PT_AMD_NO_SWEEP:
    // thirteen instances in the gem scene, ten nodes per walk) lost 15 % (profiles/r5_experiments.md section 2).
    const uint32_t top_evict = tuned(tn.top_evict_below, blob[PT_HDR_INSTANCE_COUNT] > PT_SWEEP_MAX_BITS && !scene_has_mesh(blob) ? kTopEvictBelow : 1u);
    // The grouped mesh sweep's group loop is left by a wave's last lanes (mesh_walk, GROUPS) where every parked ray of the closest-hit kernel stands in the SAME mesh — one
    // walked mesh in the table: a resumed wave is then always one the grouped sweep takes, and a ray that comes back with groups to do is never walked from the top.
    uint32_t group_evict = 1u;
    if (parked) {
        uint32_t walked = 0;
        for (uint32_t j = 0; j < blob[PT_HDR_SWEEP_COUNT]; ++j) walked += (blob[blob[PT_HDR_SWEEP_OFF] + j * PT_SWEEP_INST_WORDS + 1] & PT_SWEEP_WALKED) ? 1u : 0u;
        if (walked == 1u) group_evict = tuned(tn.group_evict_below, kGroupEvictBelow);
    }
    p.walk_policy = tuned(tn.walk_evict_below, kWalkEvictBelow) | tuned(tn.walk_search_below, kWalkSearchBelow) << 8
                  | ((tn.flags & PT_TUNE_NO_AXIS_SCAN) ? 0u : PT_WALK_SCAN_AXIS)
                  | (top_evict <= 1u ? 0u : top_evict << 24)   // (1 = never: 0 in the policy word)
                  | (group_evict <= 1u ? 0u : group_evict << 17);

    // ---- the vertex form, and what hangs on the pair of forms
    // light samples can pick the environment only if env_sampling_probability > 0: otherwise k_shade is the form without that branch
    float env_prob; std::memcpy(&env_prob, &blob[PT_HDR_ENV_PROB], sizeof env_prob);
    bool has_ggx = false;   // (a PassthroughFilter lives in the forms that hold the GGX code)
    for (uint32_t i = 0; i < blob[PT_HDR_MATERIAL_COUNT]; ++i) {
        const uint32_t kind = blob[blob[PT_HDR_MATERIAL_OFF] + i * PT_MAT_WORDS + PT_MAT_KIND];
        has_ggx = has_ggx || kind == PT_MATERIAL_GGX || kind == PT_MATERIAL_PASSTHROUGH;
    }
    // (a scene with a convex-body certificate takes at least the NO_ENV form: the lean and fused forms are compiled without the certificate code, pt_kern_shade.hip)
    p.certs = !rd.medium_aware && (flags & PT_FLAG_CONVEX) != 0u;
    p.shade_form = rd.medium_aware ? PT_SHADE_MEDIUM
                 : (env_prob != 0.0f || tn.shade_form == 2 || routed) ? PT_SHADE_FULL : (has_ggx || p.certs || tn.shade_form == 1) ? PT_SHADE_NO_ENV : PT_SHADE_LEAN;
    const bool lean = p.shade_form == PT_SHADE_LEAN;
    // (the plain light-sample kernel walks the list of live items; the parked forms list their live RAYS themselves, the measurement forms read every item)
    p.live_list = ((p.trav_form == PT_FORM_SWEEP || p.trav_form == PT_FORM_WALK || p.trav_form == PT_FORM_ANY) && lean && !(tn.flags & PT_TUNE_NO_LIVE_LIST)) ? 1u : 0u;
    p.camera_record = p.shade_form != PT_SHADE_NO_ENV ? 1u : 0u;   // (LEAN, FULL, MEDIUM: the forms whose bounce-0 launch rebuilds the camera vertex: k_shade, pt_kernels.h)
    // k_shade that traces its own segments: exists for the pure sweep form of a fully staged, transform-free scene shaded by the lean form.
    // Measured (profiles/r3_experiments.md): C2 +4..5 % (4370 us against 2095 + 2490..2640 per bounce); with four wavelengths per path it
    // lost in round 3 (C5 996 against 1093 Msamples/s: the traversal then ran at the three waves per SIMD the wide vertex code left) and wins since round 4 (PT_FUSE_HERO).
    p.fuse = !(tn.flags & PT_TUNE_NO_FUSE) && (!p.hero || PT_FUSE_HERO) && p.trav_form == PT_FORM_SWEEP && lean && (scene.lacks & PT_SCENE_NO_XF) != 0;

    // ---- pass overlap: a render whose pass loop plans two passes or more (an adaptive one: in its first round or in a later round over every pixel) wants the second
    // set of pass buffers, the second stream and the events between the two
    const auto passes = [&](uint32_t first, uint32_t count) { return plan_passes((uint32_t)ask.n_pixels, first, count, p.capacity, rd.phase_samples).size(); };
    p.overlap = !(tn.flags & PT_TUNE_NO_PASS_OVERLAP)
             && (passes(rd.first_sample, adaptive ? rd.spp : rd.sample_count) >= 2
                 || (adaptive && adaptive->max_samples > rd.spp && passes(rd.spp, std::min(adaptive->step, adaptive->max_samples - rd.spp)) >= 2));
    return true;
}

ptd::CameraParams camera_params(const pt_camera& c, float aspect_ratio) {
    using namespace ptd;
    CameraParams cam;
    F3 look_from = f3(c.look_from[0], c.look_from[1], c.look_from[2]);
    F3 look_at = f3(c.look_at[0], c.look_at[1], c.look_at[2]);
    F3 v_up = normalize(f3(c.v_up[0], c.v_up[1], c.v_up[2]));          // src/parsing/cameras.rs:139
    F3 direction = normalize(sub(look_at, look_from));
    cam.kind = c.kind; cam.span_x = cam.span_y = 0.0f; cam.w = f3(0.0f, 0.0f, 0.0f);
    if (c.kind == PT_CAMERA_PANORAMA) {  // PanoramaCamera::new (src/camera/panorama_camera.rs:18-62)
        F3 w = direction, u = normalize(cross(v_up, w)), v = normalize(cross(w, u));
        cam.origin = look_from; cam.u = u; cam.v = v; cam.w = w;
        cam.span_x = pt_clamp(c.fov[0] * 0.017453292519943295f, 0.0f, 6.283185307179586f);
        cam.span_y = pt_clamp(c.fov[1] * 0.017453292519943295f, 0.0f, 3.141592653589793f);
        cam.lower_left = cam.horizontal = cam.vertical = f3(0.0f, 0.0f, 0.0f); cam.aperture_diameter = 0.0f;
        return cam;
    }
    float theta = c.vfov * 0.017453292519943295f;                      // f32::to_radians
    float half_height = std::tan(theta / 2.0f);
    float half_width = aspect_ratio * half_height;
    F3 w = neg(direction);
    F3 u = neg(normalize(cross(v_up, w)));
    F3 v = normalize(cross(w, u));
    cam.origin = look_from; cam.u = u; cam.v = v;
    cam.lower_left = sub(sub(sub(look_from, mul(mul(u, half_width), c.focal_distance)), mul(mul(v, half_height), c.focal_distance)),
                         mul(w, c.focal_distance));
    cam.horizontal = mul(mul(mul(u, 2.0f), half_width), c.focal_distance);
    cam.vertical = mul(mul(mul(v, 2.0f), half_height), c.focal_distance);
    cam.aperture_diameter = c.aperture_diameter;
    return cam;
}

bool normalize_render_desc(const pt_render_desc& in, uint32_t camera_count, pt_render_desc* out, std::string* error) {
    pt_render_desc rd = in;
    if (rd.tile_width == 0) rd.tile_width = 32;
    if (rd.tile_height == 0) rd.tile_height = 32;
    if (rd.hero_wavelengths == 0) rd.hero_wavelengths = 1;
    if (rd.phase_samples == 0) rd.phase_samples = 10;
    if (rd.sample_count == 0) { rd.first_sample = 0; rd.sample_count = rd.spp; }
    if (rd.width == 0 || rd.height == 0 || rd.spp == 0) { *error = "width, height and spp must be positive"; return false; }
    if ((uint64_t)rd.width * rd.height > 0xffffffffull) { *error = "film too large"; return false; }
    if (rd.camera_index >= camera_count) { *error = "camera_index out of range"; return false; }
    if (rd.shard_count > 0 && rd.shard_index >= rd.shard_count) { *error = "shard_index >= shard_count"; return false; }
    if (rd.light_samples > PT_MAX_LIGHT_SAMPLES) { *error = "light_samples > 8 is not supported"; return false; }
    if (rd.hero_wavelengths != 1 && rd.hero_wavelengths != 4) { *error = "hero_wavelengths must be 1 or 4"; return false; }
    if (rd.first_sample + rd.sample_count > rd.spp) { *error = "sample range exceeds spp"; return false; }
    if (!(rd.wavelength_hi >= rd.wavelength_lo)) { *error = "bad wavelength bounds"; return false; }
    if (rd.max_bounces > 64) { *error = "max_bounces > 64"; return false; }
    if (rd.medium_aware && rd.hero_wavelengths != 1) { *error = "the medium-aware walk carries one wavelength"; return false; }
    *out = rd;
    return true;
}

pt_status normalize_adaptive_desc(const pt_render_desc& in, const pt_adaptive_desc& adaptive, bool has_sample_counts, uint32_t camera_count,
                                  pt_render_desc* out, pt_adaptive_desc* adaptive_out, std::string* error) {
    pt_adaptive_desc a = adaptive;
    if (a.step == 0) a.step = in.spp;
    if (!has_sample_counts) { *error = "sample_counts is required"; return PT_ERR_INVALID_ARGUMENT; }
    // (the NaiveRenderer's one phase of every sample cannot be extended by rounds)
    if (in.phase_samples != 0 && in.phase_samples != 10) { *error = "adaptive sampling needs phases of 10 samples (phase_samples 0 or 10)"; return PT_ERR_UNSUPPORTED; }
    if (in.shard_count != 0) { *error = "adaptive sampling deals the film's tiles itself (shard_count 0; pt_render_adaptive_multi for several devices)"; return PT_ERR_UNSUPPORTED; }
    if (in.first_sample != 0 || in.sample_count != 0) { *error = "adaptive sampling renders the whole sample range (first_sample 0, sample_count 0)"; return PT_ERR_INVALID_ARGUMENT; }
    if (in.spp % 10 != 0 || a.step % 10 != 0 || a.max_samples % 10 != 0) { *error = "spp, step and max_samples must be multiples of 10"; return PT_ERR_INVALID_ARGUMENT; }
    if (a.max_samples < in.spp) { *error = "max_samples < spp"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(a.rel_error >= 0.0f) || !(a.abs_error >= 0.0f)) { *error = "rel_error and abs_error must be >= 0"; return PT_ERR_INVALID_ARGUMENT; }
    pt_render_desc rd;
    if (!normalize_render_desc(in, camera_count, &rd, error)) return PT_ERR_INVALID_ARGUMENT;
    *out = rd;
    *adaptive_out = a;
    return PT_OK;
}

pt_status normalize_denoise_desc(const pt_denoise_desc* in, const void* film, const void* sample_counts, const void* stats, const void* guides, const void* out_film,
                                 pt_denoise_desc* out, std::string* error) {
    if (!in || !film || !sample_counts || !stats || !guides || !out_film) { *error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    pt_denoise_desc d = *in;
    if (d.width == 0 || d.height == 0) { *error = "width and height must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)d.width * (uint64_t)d.height > 0x7fffffffull) { *error = "width x height must fit 31 bits"; return PT_ERR_INVALID_ARGUMENT; }
    if (d.reserved[0] != 0) { *error = "reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (d.iterations > (uint32_t)ptd::DN_MAX_ITERATIONS) { *error = "iterations: at most 10"; return PT_ERR_INVALID_ARGUMENT; }
    if (d.normal_power_log2 > (uint32_t)ptd::DN_MAX_NORMAL_POWER_LOG2) { *error = "normal_power_log2: at most 10"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(d.sigma_luminance >= 0.0f) || !pt_isfinite(d.sigma_luminance)) { *error = "sigma_luminance must be finite and >= 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(d.sigma_depth >= 0.0f) || !pt_isfinite(d.sigma_depth)) { *error = "sigma_depth must be finite and >= 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (d.iterations == 0) d.iterations = (uint32_t)ptd::DN_DEFAULT_ITERATIONS;
    if (d.normal_power_log2 == 0) d.normal_power_log2 = (uint32_t)ptd::DN_DEFAULT_NORMAL_POWER_LOG2;
    if (d.sigma_luminance == 0.0f) d.sigma_luminance = DN_DEFAULT_SIGMA_LUMINANCE;
    if (d.sigma_depth == 0.0f) d.sigma_depth = DN_DEFAULT_SIGMA_DEPTH;
    *out = d;
    return PT_OK;
}

pt_status check_denoise_counts(size_t np, const uint32_t* sample_counts, std::string* error) {
    for (size_t p = 0; p < np; ++p)
        if (sample_counts[p] < 2u) { *error = "a sample count below 2: the variance of a mean needs two samples"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}
pt_status check_denoise_guides(size_t np, const float* guides, std::string* error) {
    for (size_t i = 0; i < 4 * np; ++i)
        if (!pt_isfinite(guides[i])) { *error = "a guide value is not finite"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}
pt_status check_denoise_inputs(const pt_denoise_desc& d, const uint32_t* sample_counts, const float* guides, std::string* error) {
    const size_t np = (size_t)d.width * d.height;
    const pt_status st = check_denoise_counts(np, sample_counts, error);
    return st != PT_OK ? st : check_denoise_guides(np, guides, error);
}

pt_status check_guides_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const void* guides, std::string* error) {
    if (!scene || !rd || !guides) { *error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    if (guide_samples == 0) { *error = "guide_samples must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (rd->width == 0 || rd->height == 0 || rd->camera_index >= camera_count) { *error = "width, height must be positive, camera_index in range"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(rd->wavelength_hi >= rd->wavelength_lo)) { *error = "wavelength_hi must not be below wavelength_lo"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)rd->width * (uint64_t)rd->height > 0x7fffffffull) { *error = "width x height must fit 31 bits"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_denoise_albedo(const pt_denoise_desc& d, const float* albedo, std::string* error) {
    const size_t np = (size_t)d.width * d.height;
    for (size_t i = 0; i < 4 * np; ++i)
        if (!pt_isfinite(albedo[i]) || !(albedo[i] >= 0.0f)) { *error = "an albedo value is not finite or is negative"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_albedo_basis_args(const pt_render_desc* rd, const void* lambda, const void* xyz, std::string* error) {
    if (!rd || !lambda || !xyz) { *error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(rd->wavelength_hi >= rd->wavelength_lo)) { *error = "wavelength_hi must not be below wavelength_lo"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_guides_chain_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                  const void* guides, pt_guide_chain_desc* out, std::string* error) {
    if (!chain) { *error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    static_assert((int)ptd::DN_CHAIN_MAX == PT_GUIDE_CHAIN_MAX, "the rules' cap is the header's");
    if (chain->max_chain > (uint32_t)PT_GUIDE_CHAIN_MAX) { *error = "max_chain: at most 16"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(chain->alpha_max >= 0.0f) || !pt_isfinite(chain->alpha_max)) { *error = "alpha_max must be finite and >= 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (chain->reserved[0] != 0 || chain->reserved[1] != 0) { *error = "reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_guides_args(scene, rd, camera_count, guide_samples, guides, error);
    if (st != PT_OK) return st;
    *out = *chain;
    if (out->alpha_max == 0.0f) out->alpha_max = DN_CHAIN_DEFAULT_ALPHA_MAX;
    return PT_OK;
}

pt_status check_matte_args(const void* scene, const pt_render_desc* rd, const pt_matte_desc* matte, uint32_t camera_count, std::string* error) {
    auto refuse = [&](const char* m) { *error = m; return PT_ERR_INVALID_ARGUMENT; };
    if (!matte) return refuse("matte: the matte desc is null");
    if (matte->samples == 0 || matte->samples > ptd::MATTE_SAMPLES_MAX) return refuse("samples must be in 1..65535");
    if (matte->ranks == 0 || matte->ranks > (uint32_t)PT_MATTE_RANKS_MAX) return refuse("ranks must be in 1..8");
    if (matte->key != (uint32_t)PT_MATTE_KEY_INSTANCE && matte->key != (uint32_t)PT_MATTE_KEY_MATERIAL) return refuse("key must be PT_MATTE_KEY_INSTANCE or PT_MATTE_KEY_MATERIAL");
    if (matte->reserved[0] != 0) return refuse("pt_matte_desc::reserved must be 0");
    if (!scene) return refuse("the scene is null");
    if (!rd) return refuse("desc: the render desc is null");
    if (rd->width == 0 || rd->height == 0) return refuse("width and height must be positive");
    if (rd->camera_index >= camera_count) return refuse("camera_index out of range");
    if (!(rd->wavelength_hi >= rd->wavelength_lo)) return refuse("wavelength_hi must not be below wavelength_lo");
    if ((uint64_t)rd->width * (uint64_t)rd->height > 0x7fffffffull) return refuse("width x height must fit 31 bits");
    return PT_OK;
}

pt_status check_matte_selections(uint32_t set_count, const uint32_t* offsets, const uint32_t* selected, const void* out, std::string* error) {
    auto refuse = [&](const char* m) { *error = m; return PT_ERR_INVALID_ARGUMENT; };
    if (set_count > ptd::MATTE_SETS_MAX) return refuse("set_count: at most 16 selections");
    if (!offsets) return refuse("offsets is null");
    if (offsets[0] != 0) return refuse("offsets must start at 0");
    for (uint32_t m = 0; m < set_count; ++m) if (offsets[m + 1] < offsets[m]) return refuse("offsets must not fall");
    if (offsets[set_count] > ptd::MATTE_SELECTED_MAX) return refuse("selected: at most 1024 keys in all");
    if (offsets[set_count] != 0 && !selected) return refuse("selected is null");
    if (set_count != 0 && !out) return refuse("out is null");
    return PT_OK;
}

pt_status check_matte_extract_args(uint32_t width, uint32_t height, uint32_t ranks, const void* keys, const void* coverage, uint32_t set_count, const uint32_t* offsets,
                                   const uint32_t* selected, const void* out, std::string* error) {
    auto refuse = [&](const char* m) { *error = m; return PT_ERR_INVALID_ARGUMENT; };
    if (width == 0 || height == 0 || (uint64_t)width * (uint64_t)height > 0x7fffffffull) return refuse("width and height must be positive and width x height must fit 31 bits");
    if (ranks == 0 || ranks > (uint32_t)PT_MATTE_RANKS_MAX) return refuse("ranks must be in 1..8");
    if (!keys || !coverage) return refuse("keys and coverage are required");
    return check_matte_selections(set_count, offsets, selected, out, error);
}

void matte_selection_words(uint32_t set_count, const uint32_t* offsets, const uint32_t* selected, std::vector<uint32_t>* words) {
    words->assign(ptd::MATTE_SETS_MAX + 1u, 0u);
    for (uint32_t m = 0; m < set_count; ++m) {
        std::vector<uint32_t> set(selected + offsets[m], selected + offsets[m + 1]);
        std::sort(set.begin(), set.end());
        set.erase(std::unique(set.begin(), set.end()), set.end());
        words->insert(words->end(), set.begin(), set.end());
        (*words)[m + 1] = (uint32_t)words->size() - (ptd::MATTE_SETS_MAX + 1u);
    }
    for (uint32_t m = set_count + 1u; m <= ptd::MATTE_SETS_MAX; ++m) (*words)[m] = (*words)[set_count];
}

pt_status check_spectral_desc(const pt_spectral_desc* sd, std::string* error) {
    if (!sd) { *error = "the spectral desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (sd->bins == 0) { *error = "bins must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (sd->bins > PT_SPECTRAL_MAX_BINS) { *error = "bins: at most 64"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t r : sd->reserved) if (r != 0) { *error = "pt_spectral_desc::reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_spectral_args(const void* scene, const pt_render_desc* rd, const pt_spectral_desc* sd, const void* film, const void* spectral, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_spectral_desc(sd, error);
    if (st != PT_OK) return st;
    if (!film) { *error = "film_xyzw is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!spectral) { *error = "the spectral film is null"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status spectral_bin_centres(const pt_render_desc* rd, const pt_spectral_desc* sd, float* centres_nm, std::string* error) {
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_spectral_desc(sd, error);
    if (st != PT_OK) return st;
    if (!centres_nm) { *error = "centres_nm is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(rd->wavelength_hi >= rd->wavelength_lo)) { *error = "bad wavelength bounds"; return PT_ERR_INVALID_ARGUMENT; }
    const float w = (rd->wavelength_hi - rd->wavelength_lo) / (float)sd->bins;
    for (uint32_t b = 0; b < sd->bins; ++b) centres_nm[b] = rd->wavelength_lo + ((float)b + 0.5f) * w;
    return PT_OK;
}

pt_status check_adaptive_spectral_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_spectral_desc* sd, uint32_t camera_count,
                                       const void* film, const void* sample_counts, const void* spectral, pt_render_desc* rd_out, pt_adaptive_desc* ad_out,
                                       std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!ad) { *error = "the adaptive desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_spectral_desc(sd, error);
    if (st != PT_OK) return st;
    if (!film) { *error = "film_xyzw is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!spectral) { *error = "the spectral film is null"; return PT_ERR_INVALID_ARGUMENT; }
    return normalize_adaptive_desc(*rd, *ad, sample_counts != nullptr, camera_count, rd_out, ad_out, error);
}

pt_status check_spectral_multi_args(const void* scene, const pt_render_desc* rd, const pt_spectral_desc* sd, uint32_t camera_count, const void* film, const void* spectral,
                                    pt_render_desc* rd_out, std::string* error) {
    const pt_status st = check_spectral_args(scene, rd, sd, film, spectral, error);
    if (st != PT_OK) return st;
    if (rd->shard_count != 0) { *error = "pt_render_spectral_multi deals the film's tiles itself: shard_count must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (!normalize_render_desc(*rd, camera_count, rd_out, error)) return PT_ERR_INVALID_ARGUMENT;
    return PT_OK;
}

pt_status check_denoise_spectral_args(const pt_denoise_desc* in, uint32_t bins, const void* film, const uint32_t* sample_counts, const void* stats, const float* guides,
                                      const void* spectral, const void* out_film, const void* out_spectral, pt_denoise_desc* out, std::string* error) {
    if (bins == 0) { *error = "bins must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (bins > PT_SPECTRAL_MAX_BINS) { *error = "bins: at most 64"; return PT_ERR_INVALID_ARGUMENT; }
    if (!spectral) { *error = "the spectral film is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!out_spectral) { *error = "out_spectral is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = normalize_denoise_desc(in, film, sample_counts, stats, guides, out_film, out, error);
    if (st != PT_OK) return st;
    return check_denoise_inputs(*out, sample_counts, guides, error);
}

pt_status check_guides_bin_albedo_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                       uint32_t bins, const void* guides, const void* bin_albedo, pt_guide_chain_desc* chain_out, std::string* error) {
    if (bins == 0) { *error = "bins must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (bins > PT_SPECTRAL_MAX_BINS) { *error = "bins: at most 64"; return PT_ERR_INVALID_ARGUMENT; }
    if (!bin_albedo) { *error = "bin_albedo is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (chain) return check_guides_chain_args(scene, rd, camera_count, guide_samples, chain, guides, chain_out, error);
    chain_out->max_chain = 0; chain_out->alpha_max = DN_CHAIN_DEFAULT_ALPHA_MAX; chain_out->reserved[0] = 0; chain_out->reserved[1] = 0;
    return check_guides_args(scene, rd, camera_count, guide_samples, guides, error);
}

pt_status check_denoise_spectral_albedo_args(const pt_denoise_desc* in, uint32_t bins, const void* film, const uint32_t* sample_counts, const void* stats,
                                             const float* guides, const float* albedo, const void* spectral, const float* bin_albedo, const void* out_film,
                                             const void* out_spectral, pt_denoise_desc* out, std::string* error) {
    pt_status st = check_denoise_spectral_args(in, bins, film, sample_counts, stats, guides, spectral, out_film, out_spectral, out, error);
    if (st == PT_OK && albedo) st = check_denoise_albedo(*out, albedo, error);
    if (st != PT_OK) return st;
    if (bin_albedo) return check_denoise_bin_albedo((size_t)bins * out->width * out->height, bin_albedo, error);
    return PT_OK;
}
pt_status check_denoise_bin_albedo(size_t n, const float* bin_albedo, std::string* error) {
    for (size_t i = 0; i < n; ++i)
        if (!pt_isfinite(bin_albedo[i]) || !(bin_albedo[i] >= 0.0f)) { *error = "a bin_albedo value is not finite or is negative"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_spectral_matrix(uint32_t K, uint32_t bins, const float* matrix, std::string* error) {
    if (!matrix) { *error = "the response matrix is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (K == 0) { *error = "K must be positive: a development needs a response"; return PT_ERR_INVALID_ARGUMENT; }
    if (K > PT_SPECTRAL_MAX_RESPONSES) { *error = "K: at most 16 responses"; return PT_ERR_INVALID_ARGUMENT; }
    if (bins == 0) { *error = "bins must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (bins > PT_SPECTRAL_MAX_BINS) { *error = "bins: at most 64"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t i = 0; i < K * bins; ++i)
        if (!pt_isfinite(matrix[i])) { *error = "a response matrix entry is not finite"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

// ---- include/pt_resident.h
pt_status check_resident_info_args(const void* scene, const void* info, std::string* error) {
    if (!scene) { *error = "pt_resident_info: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!info) { *error = "pt_resident_info: info is null"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_resident_guides_args(const void* scene, const pt_render_desc* rd, uint32_t camera_count, uint32_t guide_samples, const pt_guide_chain_desc* chain,
                                     uint32_t flags, const struct pt_resident_info& now, pt_guide_chain_desc* chain_out, std::string* error) {
    if (!scene) { *error = "pt_resident_guides: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "pt_resident_guides: the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (flags & ~(PT_RESIDENT_ALBEDO | PT_RESIDENT_BIN_ALBEDO)) { *error = "pt_resident_guides: flags holds a bit that is neither PT_RESIDENT_ALBEDO nor PT_RESIDENT_BIN_ALBEDO"; return PT_ERR_INVALID_ARGUMENT; }
    if ((flags & PT_RESIDENT_BIN_ALBEDO) && !(flags & PT_RESIDENT_ALBEDO)) { *error = "pt_resident_guides: PT_RESIDENT_BIN_ALBEDO needs PT_RESIDENT_ALBEDO"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(now.parts & PT_RESIDENT_FILM)) { *error = "pt_resident_guides: the scene has no resident film: pt_render_adaptive, pt_render_adaptive_spectral or pt_resident_load must have succeeded on it"; return PT_ERR_INVALID_ARGUMENT; }
    if (rd->width != now.width || rd->height != now.height) { *error = "pt_resident_guides: the desc's width and height are not the resident film's"; return PT_ERR_INVALID_ARGUMENT; }
    if ((flags & PT_RESIDENT_BIN_ALBEDO) && !(now.parts & PT_RESIDENT_BINS)) { *error = "pt_resident_guides: PT_RESIDENT_BIN_ALBEDO needs resident bins"; return PT_ERR_INVALID_ARGUMENT; }
    if (chain) return check_guides_chain_args(scene, rd, camera_count, guide_samples, chain, scene, chain_out, error);
    chain_out->max_chain = 0; chain_out->alpha_max = DN_CHAIN_DEFAULT_ALPHA_MAX; chain_out->reserved[0] = 0; chain_out->reserved[1] = 0;
    return check_guides_args(scene, rd, camera_count, guide_samples, scene, error);   // (the guides' destination is the scene's own: never null)
}

pt_status check_resident_load_args(const void* scene, uint32_t width, uint32_t height, uint32_t bins, const float* film, const uint32_t* sample_counts, const double* stats,
                                   const float* spectral, const float* guides, const float* albedo, const float* bin_albedo, const struct pt_resident_info& now,
                                   std::string* error) {
    if (!scene) { *error = "pt_resident_load: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!film && !sample_counts && !stats && !spectral && !guides && !albedo && !bin_albedo) { *error = "pt_resident_load: every array is null: nothing to load"; return PT_ERR_INVALID_ARGUMENT; }
    if (width == 0 || height == 0) { *error = "pt_resident_load: width and height must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) { *error = "pt_resident_load: width x height must fit 31 bits"; return PT_ERR_INVALID_ARGUMENT; }
    if ((film || sample_counts || stats) && !(film && sample_counts && stats)) { *error = "pt_resident_load: film_xyzw, sample_counts and stats come together"; return PT_ERR_INVALID_ARGUMENT; }
    if ((spectral || bin_albedo) && bins == 0) { *error = "pt_resident_load: spectral and bin_albedo need a positive bins"; return PT_ERR_INVALID_ARGUMENT; }
    if ((spectral || bin_albedo) && bins > PT_SPECTRAL_MAX_BINS) { *error = "pt_resident_load: bins: at most 64"; return PT_ERR_INVALID_ARGUMENT; }
    // what stays resident: every part that is not replaced; the denoised parts go
    uint32_t stays = now.parts & ~(PT_RESIDENT_DENOISED | PT_RESIDENT_DENOISED_BINS);
    if (film) stays &= ~PT_RESIDENT_FILM;
    if (spectral) stays &= ~PT_RESIDENT_BINS;
    if (guides) stays &= ~PT_RESIDENT_GUIDES;
    if (albedo) stays &= ~PT_RESIDENT_ALBEDO;
    if (bin_albedo) stays &= ~PT_RESIDENT_BIN_ALBEDO;
    if (stays && (width != now.width || height != now.height)) { *error = "pt_resident_load: width and height are not those of the parts that stay resident"; return PT_ERR_INVALID_ARGUMENT; }
    if ((spectral || bin_albedo) && (stays & (PT_RESIDENT_BINS | PT_RESIDENT_BIN_ALBEDO)) && bins != now.bins) { *error = "pt_resident_load: bins is not that of the planes that stay resident"; return PT_ERR_INVALID_ARGUMENT; }
    const size_t np = (size_t)width * height;
    pt_denoise_desc d;
    memset(&d, 0, sizeof(d));
    d.width = width; d.height = height;
    pt_status st = PT_OK;
    if (sample_counts) st = check_denoise_counts(np, sample_counts, error);
    if (st == PT_OK && guides) st = check_denoise_guides(np, guides, error);
    if (st == PT_OK && albedo) st = check_denoise_albedo(d, albedo, error);
    if (st == PT_OK && bin_albedo) st = check_denoise_bin_albedo((size_t)bins * np, bin_albedo, error);
    return st;
}

pt_status check_resident_denoise_args(const void* scene, const pt_resident_denoise_desc* desc, const void* out_spectral, const struct pt_resident_info& now,
                                      pt_denoise_desc* out, std::string* error) {
    if (!scene) { *error = "pt_denoise_resident: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!desc) { *error = "pt_denoise_resident: the desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (desc->flags & ~PT_RESIDENT_PLANAR_GATHER) { *error = "pt_denoise_resident: flags holds a bit that is not PT_RESIDENT_PLANAR_GATHER"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t r : desc->reserved) if (r != 0) { *error = "pt_resident_denoise_desc::reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if ((desc->filter.width == 0) != (desc->filter.height == 0)) { *error = "pt_denoise_resident: width and height are both 0 or both the resident size"; return PT_ERR_INVALID_ARGUMENT; }
    pt_denoise_desc f = desc->filter;
    const bool sized = f.width != 0;
    if (!sized) { f.width = 1; f.height = 1; }
    const pt_status st = normalize_denoise_desc(&f, scene, scene, scene, scene, scene, out, error);   // (its arrays are the scene's own: never null)
    if (st != PT_OK) return st;
    if (!(now.parts & PT_RESIDENT_FILM)) { *error = "pt_denoise_resident: the scene has no resident film: pt_render_adaptive, pt_render_adaptive_spectral or pt_resident_load must have succeeded on it"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(now.parts & PT_RESIDENT_GUIDES)) { *error = "pt_denoise_resident: the scene has no resident guides: pt_resident_guides or pt_resident_load must have succeeded on it"; return PT_ERR_INVALID_ARGUMENT; }
    if (sized && (f.width != now.width || f.height != now.height)) { *error = "pt_denoise_resident: width and height are neither 0 nor the resident size"; return PT_ERR_INVALID_ARGUMENT; }
    if (out_spectral && !(now.parts & PT_RESIDENT_BINS)) { *error = "pt_denoise_resident: out_spectral without resident bins"; return PT_ERR_INVALID_ARGUMENT; }
    out->width = now.width; out->height = now.height;
    return PT_OK;
}

pt_status check_resident_project_args(const void* scene, uint32_t K, const float* matrix, const void* out, const struct pt_resident_info& now, std::string* error) {
    if (!scene) { *error = "pt_spectral_project_resident_denoised: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!out) { *error = "pt_spectral_project_resident_denoised: the developed planes (out) are null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(now.parts & PT_RESIDENT_DENOISED_BINS)) { *error = "the scene has no resident denoised bins: pt_denoise_resident must have succeeded on it with resident bins"; return PT_ERR_INVALID_ARGUMENT; }
    return check_spectral_matrix(K, now.bins, matrix, error);
}

pt_status check_resident_assemble(const void* scene, uint32_t flags, const NodeRender& node, std::string* error) {
    if (!scene) { *error = "pt_resident_assemble: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (flags & ~PT_RESIDENT_ASSEMBLE_STAGED) { *error = "pt_resident_assemble: flags holds a bit that is not PT_RESIDENT_ASSEMBLE_STAGED"; return PT_ERR_INVALID_ARGUMENT; }
    if (!node.valid) { *error = "pt_resident_assemble: the scene has no node render to assemble: pt_render_adaptive_multi or pt_render_adaptive_spectral_multi must have succeeded on it over more than one device, with no render since"; return PT_ERR_INVALID_ARGUMENT; }
    if (!node.stats) { *error = "pt_resident_assemble: the node render was made without stats: the filter needs the statistics"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_resident_read_args(const void* scene, const void* film, const void* sample_counts, const void* stats, const void* spectral, const struct pt_resident_info& now,
                                   std::string* error) {
    if (!scene) { *error = "pt_resident_read: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (film && !(now.parts & PT_RESIDENT_FILM)) { *error = "pt_resident_read: film_xyzw without a resident film"; return PT_ERR_INVALID_ARGUMENT; }
    if (sample_counts && !(now.parts & PT_RESIDENT_FILM)) { *error = "pt_resident_read: sample_counts without a resident film"; return PT_ERR_INVALID_ARGUMENT; }
    if (stats && !(now.parts & PT_RESIDENT_FILM)) { *error = "pt_resident_read: stats without a resident film"; return PT_ERR_INVALID_ARGUMENT; }
    if (spectral && !(now.parts & PT_RESIDENT_BINS)) { *error = "pt_resident_read: spectral without resident bins"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_spectral_project_args(uint32_t width, uint32_t height, uint32_t bins, uint32_t K, const float* matrix, const void* spectral, const void* out,
                                      std::string* error) {
    if (!spectral) { *error = "the spectral film is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!out) { *error = "the developed planes (out) are null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_spectral_matrix(K, bins, matrix, error);
    if (st != PT_OK) return st;
    if (width == 0 || height == 0) { *error = "width and height must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) { *error = "width x height must fit 31 bits"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_response_matrix_args(const pt_render_desc* rd, const pt_spectral_desc* sd, const void* curves, uint32_t curve_count, const void* curve_data,
                                     uint32_t curve_data_floats, uint32_t K, const int32_t* responses, int32_t filter, uint32_t subsamples, const void* matrix,
                                     std::string* error) {
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_spectral_desc(sd, error);
    if (st != PT_OK) return st;
    if (!responses) { *error = "the responses are null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!matrix) { *error = "the response matrix is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (curve_count != 0 && !curves) { *error = "curves is null with a positive curve_count"; return PT_ERR_INVALID_ARGUMENT; }
    if (curve_data_floats != 0 && !curve_data) { *error = "curve_data is null with a positive curve_data_floats"; return PT_ERR_INVALID_ARGUMENT; }
    if (K == 0) { *error = "K must be positive: a development needs a response"; return PT_ERR_INVALID_ARGUMENT; }
    if (K > PT_SPECTRAL_MAX_RESPONSES) { *error = "K: at most 16 responses"; return PT_ERR_INVALID_ARGUMENT; }
    if (subsamples == 0) { *error = "subsamples must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if (subsamples > PT_SPECTRAL_MAX_SUBSAMPLES) { *error = "subsamples: at most 16"; return PT_ERR_INVALID_ARGUMENT; }
    if (!(rd->wavelength_hi >= rd->wavelength_lo)) { *error = "bad wavelength bounds"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t k = 0; k < K; ++k) {
        const int32_t r = responses[k];
        const bool cie = r == PT_RESPONSE_CIE_X || r == PT_RESPONSE_CIE_Y || r == PT_RESPONSE_CIE_Z;
        if (!cie && (r < 0 || (uint32_t)r >= curve_count)) { *error = "response " + std::to_string(k) + " is neither a curve index nor a PT_RESPONSE_CIE constant"; return PT_ERR_INVALID_ARGUMENT; }
    }
    if (filter != PT_SPECTRAL_NO_FILTER && (filter < 0 || (uint32_t)filter >= curve_count)) { *error = "the filter is neither a curve index nor PT_SPECTRAL_NO_FILTER"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

// node_entry: null for the one-device entries; a node entry's name, whose refusal of a shard is its own
static pt_status light_groups_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, const void* film,
                                   const char* node_entry, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!gd) { *error = "the light groups desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!film) { *error = "film_xyzw is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (gd->group_count == 0 || gd->group_count > PT_LIGHT_GROUPS_MAX) { *error = "group_count must be in 1..8"; return PT_ERR_INVALID_ARGUMENT; }
    if (gd->reserved[0] != 0 || gd->reserved[1] != 0) { *error = "pt_light_groups_desc::reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (gd->instance_count != scene_instances) {
        *error = "instance_count is " + std::to_string(gd->instance_count) + ", the scene has " + std::to_string(scene_instances) + " instances";
        return PT_ERR_INVALID_ARGUMENT;
    }
    if (gd->instance_count != 0 && !gd->instance_group) { *error = "instance_group is null"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t i = 0; i < gd->instance_count; ++i)
        if (gd->instance_group[i] >= gd->group_count) {
            *error = "instance " + std::to_string(i) + " is in group " + std::to_string(gd->instance_group[i]) + ": group ids must be below group_count";
            return PT_ERR_INVALID_ARGUMENT;
        }
    if (gd->environment_group >= gd->group_count) { *error = "environment_group must be below group_count"; return PT_ERR_INVALID_ARGUMENT; }
    if (rd->hero_wavelengths == 4) { *error = "light groups carry one wavelength per path (hero_wavelengths 0 or 1)"; return PT_ERR_UNSUPPORTED; }
    if (rd->medium_aware) { *error = "light groups are not rendered by the medium-aware walk"; return PT_ERR_UNSUPPORTED; }
    if (node_entry && rd->shard_count != 0) { *error = std::string(node_entry) + " deals the tiles itself: shard_count must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (rd->shard_count > 1) { *error = "light groups render the whole film (shard_count 0 or 1)"; return PT_ERR_UNSUPPORTED; }
    if (rd->first_sample != 0 || (rd->sample_count != 0 && rd->sample_count != rd->spp)) {
        *error = "light groups render the whole sample range (first_sample 0, sample_count 0 or spp)";
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
}

pt_status check_light_groups_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, const void* film,
                                  std::string* error) {
    return light_groups_args(scene, rd, gd, scene_instances, film, nullptr, error);
}

pt_status check_path_passes_args(const void* scene, const pt_render_desc* rd, const pt_path_passes_desc* pd, const void* film, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!pd) { *error = "the path passes desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!film) { *error = "film_xyzw is null"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t r : pd->reserved) if (r != 0) { *error = "pt_path_passes_desc::reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (rd->hero_wavelengths == 4) { *error = "path passes carry one wavelength per path (hero_wavelengths 0 or 1)"; return PT_ERR_UNSUPPORTED; }
    if (rd->medium_aware) { *error = "path passes are not rendered by the medium-aware walk"; return PT_ERR_UNSUPPORTED; }
    if (rd->shard_count > 1) { *error = "path passes render the whole film (shard_count 0 or 1)"; return PT_ERR_UNSUPPORTED; }
    if (rd->first_sample != 0 || (rd->sample_count != 0 && rd->sample_count != rd->spp)) {
        *error = "path passes render the whole sample range (first_sample 0, sample_count 0 or spp)";
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
}
pt_status check_adaptive_path_passes_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_path_passes_desc* pd, uint32_t camera_count,
                                          const void* film, const void* sample_counts, pt_render_desc* rd_out, pt_adaptive_desc* ad_out, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!ad) { *error = "the adaptive desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_path_passes_args(scene, rd, pd, film, error);
    if (st != PT_OK) return st;
    return normalize_adaptive_desc(*rd, *ad, sample_counts != nullptr, camera_count, rd_out, ad_out, error);
}

pt_status check_path_exprs_args(const void* scene, const pt_render_desc* rd, const pt_path_expr_program* program, const uint8_t* instance_group, uint32_t n_instances,
                                uint32_t scene_instances, const void* film, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!program) { *error = "the path expression program is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!film) { *error = "film_xyzw is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (program->outputs == 0 || program->outputs > PT_PATH_EXPRS_MAX) { *error = "the path expression program's outputs must be in 1..8"; return PT_ERR_INVALID_ARGUMENT; }
    if (program->states == 0 || program->states > PT_PATH_EXPR_STATES_MAX) { *error = "the path expression program's states must be in 1..64"; return PT_ERR_INVALID_ARGUMENT; }
    if (program->start >= program->states) { *error = "the path expression program's start is not below its states"; return PT_ERR_INVALID_ARGUMENT; }
    if (program->environment_group >= PT_LIGHT_GROUPS_MAX) { *error = "the path expression program's environment_group must be below 8"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t q = 0; q < program->states; ++q) {
        const uint32_t* w = program->table[q];
        for (uint32_t e = 0; e < 3u; ++e)
            if (((w[0] >> (6u * e)) & 63u) >= program->states) {
                *error = "the path expression program's state " + std::to_string(q) + " has a successor that is not below its states";
                return PT_ERR_INVALID_ARGUMENT;
            }
        const uint32_t beyond = ~((1u << program->outputs) - 1u) & 0xffu;   // (a mask bit from `outputs` on would name a plane the render does not have)
        if ((w[0] >> 18) != 0u || ((w[1] | w[2] | w[3]) & (beyond * 0x01010101u)) != 0u || (w[3] >> 8) != 0u) {
            *error = "the path expression program's state " + std::to_string(q) + " sets a bit outside its successors and the masks of its outputs";
            return PT_ERR_INVALID_ARGUMENT;
        }
    }
    if (instance_group) {
        if (n_instances != scene_instances) {
            *error = "n_instances is " + std::to_string(n_instances) + ", the scene has " + std::to_string(scene_instances) + " instances";
            return PT_ERR_INVALID_ARGUMENT;
        }
        for (uint32_t i = 0; i < n_instances; ++i)
            if (instance_group[i] >= PT_LIGHT_GROUPS_MAX) {
                *error = "instance " + std::to_string(i) + " is in group " + std::to_string(instance_group[i]) + ": group ids must be below 8";
                return PT_ERR_INVALID_ARGUMENT;
            }
    } else if (n_instances != 0) { *error = "instance_group is null: n_instances must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if (rd->hero_wavelengths == 4) { *error = "path expressions carry one wavelength per path (hero_wavelengths 0 or 1)"; return PT_ERR_UNSUPPORTED; }
    if (rd->medium_aware) { *error = "path expressions are not rendered by the medium-aware walk"; return PT_ERR_UNSUPPORTED; }
    if (rd->shard_count > 1) { *error = "path expressions render the whole film (shard_count 0 or 1)"; return PT_ERR_UNSUPPORTED; }
    if (rd->first_sample != 0 || (rd->sample_count != 0 && rd->sample_count != rd->spp)) {
        *error = "path expressions render the whole sample range (first_sample 0, sample_count 0 or spp)";
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
}
pt_status check_adaptive_path_exprs_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_path_expr_program* program,
                                         const uint8_t* instance_group, uint32_t n_instances, uint32_t scene_instances, uint32_t camera_count, const void* film,
                                         const void* sample_counts, pt_render_desc* rd_out, pt_adaptive_desc* ad_out, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!ad) { *error = "the adaptive desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_path_exprs_args(scene, rd, program, instance_group, n_instances, scene_instances, film, error);
    if (st != PT_OK) return st;
    return normalize_adaptive_desc(*rd, *ad, sample_counts != nullptr, camera_count, rd_out, ad_out, error);
}

// ---- include/pt_light_groups_multi.h
pt_status check_light_groups_multi_args(const void* scene, const pt_render_desc* rd, const pt_light_groups_desc* gd, uint32_t scene_instances, uint32_t camera_count,
                                        const void* film, pt_render_desc* rd_out, std::string* error) {
    const pt_status st = light_groups_args(scene, rd, gd, scene_instances, film, "pt_render_light_groups_multi", error);
    if (st != PT_OK) return st;
    if (!normalize_render_desc(*rd, camera_count, rd_out, error)) return PT_ERR_INVALID_ARGUMENT;
    return PT_OK;
}
pt_status check_adaptive_light_groups_multi_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_light_groups_desc* gd,
                                                 uint32_t scene_instances, uint32_t camera_count, const void* film, const void* sample_counts, pt_render_desc* rd_out,
                                                 pt_adaptive_desc* ad_out, std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!ad) { *error = "the adaptive desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = light_groups_args(scene, rd, gd, scene_instances, film, "pt_render_adaptive_light_groups_multi", error);
    if (st != PT_OK) return st;
    return normalize_adaptive_desc(*rd, *ad, sample_counts != nullptr, camera_count, rd_out, ad_out, error);
}

pt_status check_light_groups_matrices(uint32_t group_count, const float* matrices, std::string* error) {
    if (group_count == 0 || group_count > PT_LIGHT_GROUPS_MAX) { *error = "group_count must be in 1..8"; return PT_ERR_INVALID_ARGUMENT; }
    if (!matrices) { *error = "the matrices are null"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t i = 0; i < 9u * group_count; ++i)
        if (!std::isfinite(matrices[i])) { *error = "matrix entry " + std::to_string(i) + " is not finite"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

pt_status check_light_groups_mix_args(uint32_t width, uint32_t height, uint32_t group_count, const void* group_films, const float* matrices, const void* out,
                                      std::string* error) {
    if (!group_films) { *error = "the group films are null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!out) { *error = "out_xyzw is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_light_groups_matrices(group_count, matrices, error);
    if (st != PT_OK) return st;
    if (width == 0 || height == 0) { *error = "width and height must be positive"; return PT_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) { *error = "width x height must fit 31 bits"; return PT_ERR_INVALID_ARGUMENT; }
    return PT_OK;
}

// ---- include/pt_light_groups_denoise.h
pt_status check_adaptive_light_groups_args(const void* scene, const pt_render_desc* rd, const pt_adaptive_desc* ad, const pt_light_groups_desc* gd, uint32_t scene_instances,
                                           uint32_t camera_count, const void* film, const void* sample_counts, pt_render_desc* rd_out, pt_adaptive_desc* ad_out,
                                           std::string* error) {
    if (!scene) { *error = "the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!rd) { *error = "the render desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!ad) { *error = "the adaptive desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    const pt_status st = check_light_groups_args(scene, rd, gd, scene_instances, film, error);
    if (st != PT_OK) return st;
    return normalize_adaptive_desc(*rd, *ad, sample_counts != nullptr, camera_count, rd_out, ad_out, error);
}

pt_status check_denoise_light_groups_args(const pt_denoise_desc* in, uint32_t group_count, const void* film, const uint32_t* sample_counts, const void* stats,
                                          const float* guides, const float* albedo, const void* group_films, const void* out_film, const void* out_group_films,
                                          pt_denoise_desc* out, std::string* error) {
    if (group_count == 0 || group_count > PT_LIGHT_GROUPS_MAX) { *error = "group_count must be in 1..8"; return PT_ERR_INVALID_ARGUMENT; }
    if (!group_films) { *error = "the group films are null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!out_group_films) { *error = "out_group_films is null"; return PT_ERR_INVALID_ARGUMENT; }
    pt_status st = normalize_denoise_desc(in, film, sample_counts, stats, guides, out_film, out, error);
    if (st == PT_OK) st = check_denoise_inputs(*out, sample_counts, guides, error);
    if (st == PT_OK && albedo) st = check_denoise_albedo(*out, albedo, error);
    return st;
}

pt_status check_resident_denoise_light_groups_args(const void* scene, const pt_resident_denoise_desc* desc, const struct pt_resident_info& now, const GroupsResident& groups,
                                                   pt_denoise_desc* out, std::string* error) {
    if (!scene) { *error = "pt_denoise_light_groups_resident: the scene is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (!desc) { *error = "pt_denoise_light_groups_resident: the desc is null"; return PT_ERR_INVALID_ARGUMENT; }
    if (desc->flags != 0) { *error = "pt_denoise_light_groups_resident: flags must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    for (uint32_t r : desc->reserved) if (r != 0) { *error = "pt_resident_denoise_desc::reserved must be 0"; return PT_ERR_INVALID_ARGUMENT; }
    if ((desc->filter.width == 0) != (desc->filter.height == 0)) { *error = "pt_denoise_light_groups_resident: width and height are both 0 or both the resident size"; return PT_ERR_INVALID_ARGUMENT; }
    pt_denoise_desc f = desc->filter;
    const bool sized = f.width != 0;
    if (!sized) { f.width = 1; f.height = 1; }
    const pt_status st = normalize_denoise_desc(&f, scene, scene, scene, scene, scene, out, error);   // (its arrays are the scene's own: never null)
    if (st != PT_OK) return st;
    if (!(now.parts & PT_RESIDENT_FILM)) { *error = "pt_denoise_light_groups_resident: the scene has no resident film: pt_render_adaptive_light_groups must have succeeded on it"; return PT_ERR_INVALID_ARGUMENT; }
    if (!groups.valid || !groups.paired || groups.width != now.width || groups.height != now.height) {
        *error = "pt_denoise_light_groups_resident: the scene has no group films of the resident film's render: pt_render_adaptive_light_groups must have succeeded on it, with no render since";
        return PT_ERR_INVALID_ARGUMENT;
    }
    if (!(now.parts & PT_RESIDENT_GUIDES)) { *error = "pt_denoise_light_groups_resident: the scene has no resident guides: pt_resident_guides or pt_resident_load must have succeeded on it"; return PT_ERR_INVALID_ARGUMENT; }
    if (sized && (f.width != now.width || f.height != now.height)) { *error = "pt_denoise_light_groups_resident: width and height are neither 0 nor the resident size"; return PT_ERR_INVALID_ARGUMENT; }
    out->width = now.width; out->height = now.height;
    return PT_OK;
}

}  // namespace pth
