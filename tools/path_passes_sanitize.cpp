// path_passes_sanitize.cpp — a stand-alone host program for a sanitizer run of the rules of path passes (csrc/pt_path_pass_rules.h):
// the state transition, the item word, the routing of vertex additions and of an item's two sums, over random walks in a heap buffer of exactly the size the
// engine allocates — pp_planes() planes of `capacity` floats, the last of them the state words — so that a class index or a slot one past a plane is a heap
// overflow the sanitizer sees.  The state plane is poisoned before every pass, as no pass clears it: a word read before its writer wrote it ends the program.
// From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/pp_sanitize tools/path_passes_sanitize.cpp && /tmp/pp_sanitize
// It prints one line per case and "ok" at the end.  A walk whose class planes do not sum to its total plane in the order the rules add them, an addition that
// lands in a class the definition does not name, or an item word with class_b apart from class_a anywhere but at d = 0 on a GGX or Passthrough vertex ends
// it with status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_path_pass_rules.h"

using namespace ptd;

namespace {
uint32_t rng = 2463534242u;
float rnd() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return (float)(rng >> 8) * (1.0f / 16777216.0f); }
F3 rnd_dir() { return f3(rnd() * 2.0f - 1.0f, rnd() * 2.0f - 1.0f, rnd() * 2.0f - 1.0f); }
constexpr uint32_t kPoison = 0xffffffffu;

// the definition, restated without the rules' helpers: the class of a vertex addition and of a light-sample ray
uint32_t want_vertex_class(uint32_t d, uint32_t k, bool hit) { return d == 0 ? (hit ? 0u : 1u) : d == 1 ? 2u + 2u * k : 3u + 2u * k; }
uint32_t want_ray_class(uint32_t d, uint32_t k, uint32_t e) { return d == 0 ? 2u + 2u * e : 3u + 2u * k; }
}  // namespace

int main() {
    const uint32_t kinds[5] = {PT_MATERIAL_LAMBERTIAN, PT_MATERIAL_GGX, PT_MATERIAL_DIFFUSE_LIGHT, PT_MATERIAL_SHARP_LIGHT, PT_MATERIAL_PASSTHROUGH};
    for (uint32_t capacity : {1u, 97u, 1024u})
        for (uint32_t light_samples : {1u, 2u, 8u})
            for (uint32_t max_bounces : {1u, 2u, 5u, 12u}) {
                std::vector<float> buffer((size_t)pp_planes() * capacity);   // the engine's energy buffer of a pass render
                float* energy = buffer.data();
                uint32_t* state = pp_state_words(energy, capacity);
                std::vector<double> want((size_t)PP_CLASSES * capacity);    // per class and slot: the additions the definition sends there, summed in f64
                uint64_t items = 0, split_items = 0;
                for (int pass = 0; pass < 3; ++pass) {
                    for (size_t i = 0; i < (size_t)lg_planes(PP_CLASSES) * capacity; ++i) energy[i] = 0.0f;
                    for (uint32_t i = 0; i < capacity; ++i) state[i] = kPoison;
                    std::fill(want.begin(), want.end(), 0.0);
                    std::vector<uint32_t> live(capacity);
                    for (uint32_t i = 0; i < capacity; ++i) live[i] = i;
                    std::vector<uint32_t> true_d(capacity, 0u), true_k(capacity, 0u);   // the walk's own history, kept apart from the packed word
                    for (uint32_t bounce = 0; bounce < max_bounces && !live.empty(); ++bounce) {
                        std::vector<uint32_t> next;
                        for (uint32_t slot : live) {
                            // PassRouter's steps of routed_vertex (pt_path_pass_rules.h, pt_routed_rules.h) over a made-up vertex
                            const uint32_t before = bounce == 0u ? 0u : state[slot];
                            if (before == kPoison) { printf("slot %u bounce %u: the state word is read before it is written\n", slot, bounce); return 1; }
                            const uint32_t d = pp_state_d(before), k = pp_state_k(before);
                            if (d != true_d[slot] || (d != 0u && k != true_k[slot])) { printf("slot %u bounce %u: the word carries (%u, %u), the walk is at (%u, %u)\n", slot, bounce, d, k, true_d[slot], true_k[slot]); return 1; }
                            const bool hit = rnd() < 0.85f;
                            const uint32_t kind = kinds[(uint32_t)(rnd() * 5.0f) % 5u];
                            const bool diffuse = hit ? pp_kind_is_diffuse(kind) : true, glossy = kind == PT_MATERIAL_GGX || kind == PT_MATERIAL_PASSTHROUGH;
                            const F3 n = rnd_dir(), in_d = rnd_dir();
                            uint32_t word = pp_item_classes(d, k, diffuse);
                            const bool has_item = hit && kind != PT_MATERIAL_DIFFUSE_LIGHT && kind != PT_MATERIAL_SHARP_LIGHT;
                            float contribution[PT_MAX_LIGHT_SAMPLES];
                            if (has_item)
                                for (uint32_t l = 0; l < light_samples; ++l) {
                                    const F3 ray_d = rnd() < 0.2f ? f3(0.0f, 0.0f, 0.0f) : rnd_dir();   // (a dead ray's direction is zero)
                                    word |= pp_item_ray_bit(d, diffuse, n, in_d, l, ray_d);
                                    contribution[l] = rnd() < 0.3f ? 0.0f : rnd();
                                    const bool same_side = (((n.x * in_d.x + n.y * in_d.y) + n.z * in_d.z) > 0.0f) == (((n.x * ray_d.x + n.y * ray_d.y) + n.z * ray_d.z) > 0.0f);
                                    const uint32_t e = diffuse ? 0u : same_side ? 2u : 1u;
                                    want[(size_t)want_ray_class(d, k, e) * capacity + slot] += (double)(contribution[l] / (float)light_samples);   // (term by term: the rules divide the class's sum once)
                                }
                            if (!hit || rnd() < 0.3f) {   // a vertex addition: an environment vertex always, a light vertex sometimes
                                const float add = rnd();
                                energy[slot] += add;
                                pp_add_vertex(d, k, hit, add, energy, capacity, slot);
                                want[(size_t)want_vertex_class(d, k, hit) * capacity + slot] += (double)add;
                            }
                            const bool survives = hit && rnd() < 0.8f && bounce + 1 < max_bounces;
                            const F3 out_d = rnd_dir();
                            uint32_t e = 0;
                            if (survives) e = pp_event_kind(diffuse, n, in_d, out_d);
                            if (hit) state[slot] = word | (survives ? pp_next_state(d, k, e) : 0u);
                            if (survives) { next.push_back(slot); true_k[slot] = d == 0u ? e : true_k[slot]; true_d[slot] = d + 1u < 2u ? d + 1u : 2u; }
                            // PassRouter's steps of routed_shadow_item: the fold and the add, reading the word back from the plane
                            if (has_item) {
                                const uint32_t w = state[slot];
                                const uint32_t a = pp_item_class_a(w), b = pp_item_class_b(w);
                                ++items;
                                if ((b != a) != (d == 0u && glossy)) { printf("slot %u bounce %u: class_b %u beside class_a %u at d = %u on kind %u\n", slot, bounce, b, a, d, kind); return 1; }
                                if (b != a) { ++split_items; if (a != 4u || b != 6u) { printf("a split item of classes %u and %u\n", a, b); return 1; } }
                                if (b == a && ((w >> 8) & 0xffu) != 0u) { printf("ray bits of class_b in an item of one class\n"); return 1; }
                                float lc = 0.0f, sum_a = 0.0f, sum_b = 0.0f;
                                for (uint32_t l = 0; l < light_samples; ++l) { lc += contribution[l]; pp_item_fold(w, l, contribution[l], &sum_a, &sum_b); }
                                energy[slot] += lc / (float)light_samples;
                                pp_item_add(w, sum_a, sum_b, light_samples, energy, capacity, slot);
                            }
                        }
                        live.swap(next);
                    }
                    // every class plane holds what the definition sends there (f32 sums of a few terms against f64: a relative 1e-5 is rounding), and the classes
                    // together hold the total
                    for (uint32_t slot = 0; slot < capacity; ++slot) {
                        double sum = 0.0;
                        for (uint32_t c = 0; c < PP_CLASSES; ++c) {
                            const double got = (double)energy[(size_t)lg_plane(c) * capacity + slot], w = want[(size_t)c * capacity + slot];
                            if (got < w - 1e-5 * (1.0 + w) || got > w + 1e-5 * (1.0 + w)) { printf("slot %u class %u: %.9g, the definition sends %.9g there\n", slot, c, got, w); return 1; }
                            sum += got;
                        }
                        const double total = (double)energy[slot];
                        if (sum < total - 1e-5 * (1.0 + total) || sum > total + 1e-5 * (1.0 + total)) { printf("slot %u: the classes hold %.9g, the total %.9g\n", slot, sum, total); return 1; }
                    }
                }
                printf("capacity %u, L = %u, %u bounces: %llu items (%llu of two classes) routed as the definition says, the classes sum to the total\n", capacity, light_samples,
                       max_bounces, (unsigned long long)items, (unsigned long long)split_items);
            }
    printf("ok\n");
    return 0;
}
