// path_exprs_sanitize.cpp — a stand-alone host program for a sanitizer run of path expressions (include/pt_light_groups.h "Path expressions"):
// the compiler and the match (csrc/pt_path_expr.cpp) over sets that compile, sets that are refused and every kind of syntax error, and the router's rules
// (csrc/pt_path_expr_rules.h) — the state word, the ray bits, the routing of vertex additions and of an item's eight sums — over random walks in a heap buffer of
// exactly the size the engine allocates: px_planes(K) planes of `capacity` floats, the last of them the state words, beside a table of exactly 64 entries, so that a
// plane index, a slot or a state one past its array is a heap overflow the sanitizer sees.  The state plane is poisoned before every pass, as no pass clears it: a
// word read before its writer wrote it ends the program.  From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unknown-pragmas -Wno-unused-function
//       -o /tmp/px_sanitize tools/path_exprs_sanitize.cpp rust-pathtracer_amd/csrc/pt_path_expr.cpp && /tmp/px_sanitize
// It prints one line per case and "ok" at the end.  A plane that does not hold what the definition sends there — every contribution's path written out and
// matched on its own — or a built-in expression that disagrees with the path passes' classes ends it with status 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/pt_path_expr_rules.h"
#include "../include/pt_light_groups.h"

using namespace ptd;

namespace {
uint32_t rng = 2463534242u;
float rnd() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return (float)(rng >> 8) * (1.0f / 16777216.0f); }
F3 rnd_dir() { return f3(rnd() * 2.0f - 1.0f, rnd() * 2.0f - 1.0f, rnd() * 2.0f - 1.0f); }
constexpr uint32_t kPoison = 0xffffffffu;

bool compile(const std::vector<const char*>& exprs, uint32_t env, pt_path_expr_program* program, pt_status want = PT_OK) {
    char err[64];   // (shorter than most messages: they are cut to it)
    const pt_status st = pt_path_expr_compile(exprs.data(), (uint32_t)exprs.size(), env, program, err, sizeof(err));
    if (st != want) { printf("compiling a set of %zu expressions gave status %d (%s), not %d\n", exprs.size(), (int)st, err, (int)want); return false; }
    return true;
}
std::string terminal_text(uint32_t t) { return t < 8u ? "L" + std::to_string(t) : std::string("E"); }
}  // namespace

int main() {
    pt_path_expr_program program;
    // ---- the compiler: the built-in expressions against the classes of the path passes, restated
    const std::vector<const char*> built_in = {"CL", "CE", "CD[LE]", "CD.+[LE]", "CR[LE]", "CR.+[LE]", "CT[LE]", "CT.+[LE]"};
    if (!compile(built_in, 0u, &program)) return 1;
    uint64_t paths = 0;
    for (uint32_t n = 0; n <= 7u; ++n)
        for (uint32_t code = 0; code < (n == 0 ? 1u : 1u << (2u * n)); ++code) {
            std::string events;
            bool ok = true;
            for (uint32_t i = 0; i < n; ++i) { const uint32_t e = (code >> (2u * i)) & 3u; ok = ok && e < 3u; events += "DRT"[e % 3u]; }
            if (!ok) continue;
            for (uint32_t t = 0; t < 9u; ++t) {
                const uint32_t k = n ? (uint32_t)std::string("DRT").find(events[0]) : 0u;
                const uint32_t cls = n == 0 ? (t < 8u ? 0u : 1u) : n == 1 ? 2u + 2u * k : 3u + 2u * k;
                uint32_t mask = 0;
                const std::string path = "C" + events + terminal_text(t);
                if (pt_path_expr_match(&program, path.c_str(), &mask) != PT_OK || mask != 1u << cls) { printf("%s: mask %#x, the path passes put it in class %u\n", path.c_str(), mask, cls); return 1; }
                ++paths;
            }
        }
    printf("the built-in expressions: %u states, %llu paths in the class the path passes name\n", program.states, (unsigned long long)paths);
    // ---- what is refused: every kind of syntax error, too many states, bad counts, malformed paths
    const char* const bad[] = {"", "DL", "CD", "CD(", "CD)L", "C(DL)", "C*L", "CD|RL", "CDxL", "CDL9", "CDLD", "CDL|", "C[DX]L", "C[^DRT]L", "C[D", "CD[LD]", "C()L", "C(D|R L", "CCL",
                               "C(D", "C[", "C[^", "CD[L", "CD[L2", "C((((D", "CL0E", "C.*+?L|", "C|L"};
    for (const char* text : bad) if (!compile({"CL", text}, 0u, &program, PT_ERR_INVALID_ARGUMENT)) return 1;
    if (!compile({"C.*D......L"}, 0u, &program, PT_ERR_UNSUPPORTED) || !compile({}, 0u, &program, PT_ERR_INVALID_ARGUMENT) || !compile({"CL"}, 8u, &program, PT_ERR_INVALID_ARGUMENT)) return 1;
    if (!compile({"C.*D.....L"}, 0u, &program) || program.states != 64u) { printf("the largest program has %u states, not 64\n", program.states); return 1; }
    uint32_t mask = 0;
    for (const char* path : {"", "C", "CD", "DL", "CDX", "CDL8", "CDLL", "CDE9", "C D L"})
        if (pt_path_expr_match(&program, path, &mask) != PT_ERR_INVALID_ARGUMENT) { printf("the malformed path \"%s\" is matched\n", path); return 1; }
    printf("%zu syntax errors, the refusals and the malformed paths\n", sizeof(bad) / sizeof(bad[0]));

    // ---- the router's rules over random walks
    const uint32_t kinds[5] = {PT_MATERIAL_LAMBERTIAN, PT_MATERIAL_GGX, PT_MATERIAL_DIFFUSE_LIGHT, PT_MATERIAL_SHARP_LIGHT, PT_MATERIAL_PASSTHROUGH};
    const std::vector<std::vector<const char*>> sets = {
        {"C.*[LE]", "CD[RT]+[LE]", "C(DR|T?D)*L1|CR+E", "C[^D]*E0", "C.*T.*T.*[LE]"}, {"C.*[LE]"}, built_in, {"C.*D.....L"}, {"C.*[L2E2]", "CT+(D|R)?[L1E1]", "C.?.?L"}};
    for (size_t which = 0; which < sets.size(); ++which)
        for (uint32_t capacity : {1u, 97u, 1024u})
            for (uint32_t light_samples : {1u, 3u, 8u}) {
                const uint32_t env = (uint32_t)which % 3u, max_bounces = which == 3 ? 12u : 6u;
                if (!compile(sets[which], env, &program)) return 1;
                const uint32_t K = program.outputs;
                std::vector<PxEntry> table(PX_MAX_STATES, PxEntry{0u, 0u, 0u, 0u});   // as the engine uploads it: the program's states, the rest zero
                for (uint32_t q = 0; q < program.states; ++q) table[q] = PxEntry{program.table[q][0], program.table[q][1], program.table[q][2], program.table[q][3]};
                std::vector<float> buffer((size_t)px_planes(K) * capacity);   // the engine's energy buffer of an expression render
                float* energy = buffer.data();
                uint32_t* state = px_state_words(energy, capacity, K);
                std::vector<double> want((size_t)K * capacity);    // per expression and slot: the additions the definition sends there, summed in f64
                uint64_t items = 0, routed = 0;
                for (int pass = 0; pass < 2; ++pass) {
                    for (size_t i = 0; i < (size_t)lg_planes(K) * capacity; ++i) energy[i] = 0.0f;
                    for (uint32_t i = 0; i < capacity; ++i) state[i] = kPoison;
                    std::fill(want.begin(), want.end(), 0.0);
                    std::vector<uint32_t> live(capacity);
                    for (uint32_t i = 0; i < capacity; ++i) live[i] = i;
                    std::vector<std::string> written(capacity, "C");   // the walk's own history, kept apart from the packed word
                    const auto send = [&](const std::string& path, uint32_t slot, double value) -> bool {
                        uint32_t m = 0;
                        if (pt_path_expr_match(&program, path.c_str(), &m) != PT_OK) { printf("the path %s is refused\n", path.c_str()); return false; }
                        for (uint32_t e = 0; e < K; ++e) if ((m >> e) & 1u) { want[(size_t)e * capacity + slot] += value; ++routed; }
                        return true;
                    };
                    for (uint32_t bounce = 0; bounce < max_bounces && !live.empty(); ++bounce) {
                        std::vector<uint32_t> next;
                        for (uint32_t slot : live) {
                            // ExprRouter's steps of routed_vertex (pt_path_expr_rules.h, pt_routed_rules.h) over a made-up vertex
                            const uint32_t before = bounce == 0u ? 0u : state[slot];
                            if (before == kPoison) { printf("slot %u bounce %u: the state word is read before it is written\n", slot, bounce); return 1; }
                            const PxState q = px_state(table[bounce == 0u ? program.start : px_word_behind(before)]);
                            const bool hit = rnd() < 0.85f;
                            const uint32_t kind = kinds[(uint32_t)(rnd() * 5.0f) % 5u], group = (uint32_t)(rnd() * 8.0f) % 8u;
                            const bool diffuse = hit ? pp_kind_is_diffuse(kind) : true;
                            const F3 n = rnd_dir(), in_d = rnd_dir();
                            uint32_t word = px_item_states(q, diffuse);
                            const bool has_item = hit && kind != PT_MATERIAL_DIFFUSE_LIGHT && kind != PT_MATERIAL_SHARP_LIGHT;
                            float contribution[PT_MAX_LIGHT_SAMPLES];
                            uint32_t ray_terminal[PT_MAX_LIGHT_SAMPLES];
                            if (has_item)
                                for (uint32_t l = 0; l < light_samples; ++l) {
                                    const F3 ray_d = rnd() < 0.2f ? f3(0.0f, 0.0f, 0.0f) : rnd_dir();   // (a dead ray's direction is zero)
                                    word |= px_item_ray_bit(diffuse, n, in_d, l, ray_d);
                                    const bool lit = rnd() < 0.5f;
                                    contribution[l] = lit || rnd() < 0.3f ? rnd() : 0.0f;   // (a ray that is not lit and adds: an environment ray that escapes)
                                    ray_terminal[l] = lit ? (uint32_t)(rnd() * 8.0f) % 8u : PX_ENVIRONMENT;
                                    const bool same_side = (((n.x * in_d.x + n.y * in_d.y) + n.z * in_d.z) > 0.0f) == (((n.x * ray_d.x + n.y * ray_d.y) + n.z * ray_d.z) > 0.0f);
                                    const char e = diffuse ? 'D' : same_side ? 'T' : 'R';
                                    // (term by term: the rules divide an expression's sum once)
                                    if (!send(written[slot] + e + terminal_text(ray_terminal[l]), slot, (double)(contribution[l] / (float)light_samples))) return 1;
                                }
                            if (!hit || rnd() < 0.3f) {   // a vertex addition: an environment vertex always, a light vertex sometimes
                                const float add = rnd();
                                const uint32_t t = hit ? group : PX_ENVIRONMENT;
                                energy[slot] += add;
                                px_add_vertex(px_mask(q, t), add, energy, capacity, slot);
                                if (!send(written[slot] + terminal_text(t), slot, (double)add)) return 1;
                            }
                            const bool survives = hit && rnd() < 0.8f && bounce + 1 < max_bounces;
                            const F3 out_d = rnd_dir();
                            uint32_t e = 0;
                            if (survives) e = pp_event_kind(diffuse, n, in_d, out_d);
                            if (hit) state[slot] = word | (survives ? px_next(q, e) << 20 : 0u);
                            if (survives) { next.push_back(slot); written[slot] += "DRT"[e]; }
                            // ExprRouter's steps of routed_shadow_item: the two entries, the fold and the add, reading the word back from the plane
                            if (has_item) {
                                const uint32_t w = state[slot];
                                const PxState entry_a = px_state(table[px_word_state_a(w)]), entry_b = px_state(table[px_word_state_b(w)]);
                                ++items;
                                float lc = 0.0f, sums[PX_MAX_EXPRS];
                                uint32_t any = 0u;
                                lg_item_clear(sums);
                                for (uint32_t l = 0; l < light_samples; ++l) {
                                    lc += contribution[l];
                                    const uint32_t m = px_word_ray_in_b(w, l) ? px_mask(entry_b, ray_terminal[l]) : px_mask(entry_a, ray_terminal[l]);
                                    any |= m;
                                    px_item_fold(sums, m, contribution[l]);
                                }
                                if (any >> K) { printf("slot %u bounce %u: a mask names an expression the program does not have\n", slot, bounce); return 1; }
                                energy[slot] += lc / (float)light_samples;
                                px_item_add(sums, any, light_samples, energy, capacity, slot);
                            }
                        }
                        live.swap(next);
                    }
                    // every expression's plane holds what the definition sends there (f32 sums of a few terms against f64: a relative 1e-5 is rounding)
                    for (uint32_t slot = 0; slot < capacity; ++slot)
                        for (uint32_t e = 0; e < K; ++e) {
                            const double got = (double)energy[(size_t)lg_plane(e) * capacity + slot], w = want[(size_t)e * capacity + slot];
                            if (got < w - 1e-5 * (1.0 + w) || got > w + 1e-5 * (1.0 + w)) { printf("set %zu slot %u expression %u: %.9g, the definition sends %.9g there\n", which, slot, e, got, w); return 1; }
                        }
                }
                printf("set %zu (%u expressions, %u states), capacity %u, L = %u: %llu items, %llu additions routed as the definition says\n", which, K, program.states, capacity,
                       light_samples, (unsigned long long)items, (unsigned long long)routed);
            }
    printf("ok\n");
    return 0;
}
