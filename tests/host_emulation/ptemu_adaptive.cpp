// ptemu_adaptive.cpp — TEST HARNESS: pt_render_adaptive (include/pt_adaptive.h) on the CPU.  Linked into the emulation library
// beside ptemu.cpp (tests/test_adaptive.py builds it); not part of the product.
//
// The driver is the engine's (pt_engine.hip adaptive_rounds): the same argument check (pth::normalize_adaptive_desc), the same round-0 list
// (pth::shard_pixels) and the same decision and keep rules (pt_adaptive_select.h).  The sample work is done by ptemu_render on ranges of ONE
// sample: such a film holds that sample's XYZ terms exactly (each is added to 0.0f), so summing them from 0.0f in sample order rebuilds each
// phase sum of stage_accumulate_pixel, and adding that onto the running film is the engine's own f32 sequence.
#include <cstring>
#include <string>
#include <vector>

#include "../../rust-pathtracer_amd/csrc/pt_adaptive_select.h"
#include "../../rust-pathtracer_amd/csrc/pt_plan.h"
#include "../../rust-pathtracer_amd/csrc/pt_scene_host.h"
#include "../../include/pt_adaptive.h"

using namespace ptd;

struct pt_scene { pth::HostScene host; };   // (ptemu.cpp's handle, the same definition)

extern "C" pt_status ptemu_render(pt_scene* sc, const pt_render_desc* rdp, float* film, pt_profile* profile);

static thread_local std::string g_adaptive_error;

// One round's mark, keep and compaction: every pixel of `list` (n entries, `count` samples each) takes the count and its decision, then the pixels
// that go on are written to `next` in list order.  The byte image is cleared first, as the engine clears it before each round.
static uint32_t select_round(uint32_t width, uint32_t height, const uint32_t* list, uint32_t n, uint32_t count, const double* stats, uint32_t max_samples,
                             float rel_error, float abs_error, uint32_t* counts, uint8_t* unconverged, uint32_t* next) {
    std::memset(unconverged, 0, (size_t)width * height);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t p = list[i];
        counts[p] = count;
        unconverged[p] = adaptive_unconverged(count, stats[2 * (size_t)p], stats[2 * (size_t)p + 1], rel_error, abs_error) ? 1u : 0u;
    }
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (adaptive_keep(unconverged, width, height, list[i], count, max_samples)) next[kept++] = list[i];
    return kept;
}

extern "C" {

const char* ptemu_adaptive_last_error(void) { return g_adaptive_error.c_str(); }

// counts: width*height (the list's pixels are set to `count`), unconverged: width*height bytes (out), next: n entries (out), *n_next: its length
pt_status ptemu_adaptive_select(uint32_t width, uint32_t height, const uint32_t* list, uint32_t n, uint32_t count, const double* stats, uint32_t max_samples,
                                float rel_error, float abs_error, uint32_t* counts, uint8_t* unconverged, uint32_t* next, uint32_t* n_next) {
    if (width == 0 || height == 0 || !list || !stats || !counts || !unconverged || !next || !n_next) return PT_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n; ++i) if (list[i] >= width * height) return PT_ERR_INVALID_ARGUMENT;
    *n_next = select_round(width, height, list, n, count, stats, max_samples, rel_error, abs_error, counts, unconverged, next);
    return PT_OK;
}

pt_status ptemu_render_adaptive(pt_scene* sc, const pt_render_desc* rdp, const pt_adaptive_desc* adp, float* film, uint32_t* sample_counts, double* stats,
                                pt_profile* profile) {
    if (!sc || !rdp || !adp || !film) { g_adaptive_error = "null argument"; return PT_ERR_INVALID_ARGUMENT; }
    pt_render_desc rd;
    pt_adaptive_desc ad;
    pt_status st = pth::normalize_adaptive_desc(*rdp, *adp, sample_counts != nullptr, (uint32_t)sc->host.cameras.size(), &rd, &ad, &g_adaptive_error);
    if (st != PT_OK) return st;
    const uint32_t w = rd.width, h = rd.height;
    const size_t np = (size_t)w * h;
    std::vector<uint32_t> lists[2];
    lists[0] = pth::shard_pixels(w, h, rd.tile_width, rd.tile_height, 0, 0);
    lists[1].resize(lists[0].size());
    std::vector<float> sum(4 * np, 0.0f), phase(3 * np, 0.0f), one(4 * np);
    std::vector<double> st2(2 * np, 0.0);
    std::vector<uint8_t> unconverged(np);
    uint32_t n = (uint32_t)lists[0].size(), c = 0, len = rd.spp, cur = 0, rounds = 0;
    uint64_t camera_rays = 0;
    for (;;) {
        const uint32_t* list = lists[cur].data();
        for (uint32_t s = c; s < c + len; ++s) {
            pt_render_desc one_rd = rd;   // one sample of the whole film (the film of a partial range is not divided)
            one_rd.spp = ad.max_samples; one_rd.first_sample = s; one_rd.sample_count = 1;
            st = ptemu_render(sc, &one_rd, one.data(), nullptr);
            if (st != PT_OK) { g_adaptive_error = "ptemu_render failed"; return st; }
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t p = list[i];
                for (int k = 0; k < 3; ++k) phase[3 * (size_t)p + k] += one[4 * (size_t)p + k];
                const double y = (double)one[4 * (size_t)p + 1];
                st2[2 * (size_t)p] += y; st2[2 * (size_t)p + 1] += y * y;
                if ((s + 1) % 10 == 0)   // (rounds end on phase boundaries)
                    for (int k = 0; k < 3; ++k) { sum[4 * (size_t)p + k] += phase[3 * (size_t)p + k]; phase[3 * (size_t)p + k] = 0.0f; }
            }
        }
        camera_rays += (uint64_t)n * len;
        c += len;
        ++rounds;
        const uint32_t kept = select_round(w, h, list, n, c, st2.data(), ad.max_samples, ad.rel_error, ad.abs_error, sample_counts, unconverged.data(),
                                           lists[cur ^ 1u].data());
        if (c >= ad.max_samples || kept == 0) break;
        n = kept;
        cur ^= 1u;
        len = ad.step < ad.max_samples - c ? ad.step : ad.max_samples - c;
    }
    for (size_t p = 0; p < np; ++p) {
        const float cnt = (float)sample_counts[p];
        film[4 * p] = sum[4 * p] / cnt; film[4 * p + 1] = sum[4 * p + 1] / cnt; film[4 * p + 2] = sum[4 * p + 2] / cnt; film[4 * p + 3] = 0.0f;
    }
    if (stats) std::memcpy(stats, st2.data(), sizeof(double) * 2 * np);
    if (profile) {
        std::memset(profile, 0, sizeof(*profile));
        profile->camera_rays = camera_rays;
        profile->kernel_launches[5] = rounds;
    }
    return PT_OK;
}

}  // extern "C"
