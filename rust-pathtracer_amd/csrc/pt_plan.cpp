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
