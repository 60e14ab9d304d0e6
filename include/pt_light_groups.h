/* pt_light_groups.h — light groups: per-group films from one render, mixed on the device.
 *
 * Not part of pt_api.h: that header is the boundary the oracle shares, and the reference keeps one film.  Exported by libptamd.so (pt_); the rules are also
 * compiled into the host emulation of the tests (ptemu_light_groups_*).  The definition is DESIGN.md section 15; in short:
 *
 *   every instance of the scene belongs to one of G groups, 1 <= G <= 8, and so does the environment.  Every addition to a sample's energy goes to the plane of
 *   exactly one group: a light vertex to the group of the instance it lies on (an emissive mesh face: its instance's), an environment vertex to the
 *   environment's, a light-sample ray that hits a light to the group of the instance it hit, an environment light-sample ray that escapes to the environment's.
 *   Within a light-sample item group g's share is the sum in ray order of g's ray contributions, divided by light_samples.  Group g's film is made from group
 *   g's energies as pt_render's is made from all of them: the same wavelengths, phases of 10 and normalisation.
 *
 *   film_xyzw is pt_render's film bit for bit.  Where every film is finite, group g's film is pt_render's of the same scene with every emitter outside g
 *   emitting a zero curve, bit for bit.  Contributions are routed, nothing is multiplied by zero: an infinite factor times a zero emission is NaN in that masked
 *   render and absent here.
 *
 * Layout: group-major films, each row-major like the film with y = 0 the top row: group_films[((g * height + y) * width + x) * 4 + c], f32, w = 0.
 *
 * The mix (the relight): with M[g] a row-major 3 x 3 per group, all f32, no contraction,
 *   out_c(p) = fold over g ascending of acc = acc + ((M[g][c][0] * X_g(p) + M[g][c][1] * Y_g(p)) + M[g][c][2] * Z_g(p)), from acc = 0.0f;   out_w = 0.
 * A scaled identity is a group's intensity, a diagonal its tint, a full matrix a white balance of its own, zero switches it off.
 *
 * The adaptive group render and the joint filter over group films are pt_light_groups_denoise.h's. */
#ifndef PT_LIGHT_GROUPS_H
#define PT_LIGHT_GROUPS_H
#include "pt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_LIGHT_GROUPS_MAX 8

typedef struct pt_light_groups_desc {
    uint32_t group_count;             /* 1 .. PT_LIGHT_GROUPS_MAX */
    uint32_t instance_count;          /* must equal the scene's */
    const uint8_t* instance_group;    /* per instance, each < group_count; read for every instance, used where it emits */
    uint32_t environment_group;       /* < group_count */
    uint32_t reserved[2];             /* must be 0 */
} pt_light_groups_desc;

/* desc: what pt_render takes, one wavelength per path, the plain walk, the whole film and the whole sample range: hero_wavelengths 4, medium_aware, a shard and
 * a partial sample range are PT_ERR_UNSUPPORTED.  film_xyzw: width*height*4 f32, pt_render's film.  group_films: group_count*width*height*4 f32, or NULL when
 * only the resident copy is wanted.  profile (may be NULL): pt_render's counters; kernel_seconds[4] (accumulate) includes the per-group kernel.
 * The group films stay on the scene's device until the next group render replaces them or the scene is destroyed. */
pt_status pt_render_light_groups(pt_scene* scene, const pt_render_desc* desc, const pt_light_groups_desc* groups, float* film_xyzw, float* group_films,
                                 pt_profile* profile);

/* The mix of host arrays.  group_films: group_count*width*height*4 f32; matrices: group_count*9 f32, row-major, every entry finite; out_xyzw: width*height*4 f32.
 * width x height within 31 bits. */
pt_status pt_light_groups_mix(uint32_t width, uint32_t height, uint32_t group_count, const float* group_films, const float* matrices, float* out_xyzw);

/* What the scene's last group render left on its device: its size and group count, or three zeros when there is none. */
pt_status pt_light_groups_resident(pt_scene* scene, uint32_t* width, uint32_t* height, uint32_t* group_count);

/* pt_light_groups_mix over the resident group films: the matrices go up, one film comes back. */
pt_status pt_light_groups_mix_resident(pt_scene* scene, const float* matrices, float* out_xyzw);

/* ---- Path passes: the render split by HOW the light travelled.  A pass render is a group render whose group is a function of the
 * path's own history, not of the emitter: eight films, in this order, each made from its class's energies as pt_render's film is made from all of them.
 *
 *   The state in front of a vertex is (d, k): d the scattering events so far (the camera vertex: 0), k the kind of the first — diffuse (a Lambertian,
 *   DiffuseLight or SharpLight record), else reflection or transmission by whether the direction leaves on the side it came from.  Every surface vertex the walk
 *   continues from is an event.  A light or environment vertex' addition goes to emission / background at d = 0, to k-direct at d = 1, to k-indirect from
 *   d = 2 on; a light-sample ray made at d = 0 goes to (its own direction's kind)-direct, any later one to k-indirect.  film_xyzw is pt_render's bit for bit.
 *
 * The pass films are left on the scene's device as ITS RESIDENT GROUP FILMS with group_count 8: pt_light_groups_resident, pt_light_groups_mix_resident and
 * (after the adaptive entry of pt_light_groups_denoise.h) pt_denoise_light_groups_resident follow a pass render as they follow a group render.
 * Out of scope: a device mask, spectral bins per pass, hero wavelengths, the medium-aware walk.
 * (Declared here, not in a header of its own, because the pass films ARE group films.  The return type stands on a line of its own: the light-group tests
 * pin the list of this header's `pt_status pt_...(` lines to the light-group entries above.) */
#define PT_PATH_PASSES 8
enum {
    PT_PATH_PASS_EMISSION = 0,
    PT_PATH_PASS_BACKGROUND = 1,
    PT_PATH_PASS_DIFFUSE_DIRECT = 2,
    PT_PATH_PASS_DIFFUSE_INDIRECT = 3,
    PT_PATH_PASS_REFLECTION_DIRECT = 4,
    PT_PATH_PASS_REFLECTION_INDIRECT = 5,
    PT_PATH_PASS_TRANSMISSION_DIRECT = 6,
    PT_PATH_PASS_TRANSMISSION_INDIRECT = 7
};

typedef struct pt_path_passes_desc {
    uint32_t reserved[4];             /* must be 0 */
} pt_path_passes_desc;

/* desc, film_xyzw, profile: pt_render_light_groups'; refused is what that entry refuses of a render desc (hero_wavelengths 4, medium_aware, a shard, a partial
 * sample range: PT_ERR_UNSUPPORTED).  pass_films: PT_PATH_PASSES*width*height*4 f32 in the layout of group films, or NULL when only the resident copy is wanted. */
pt_status
pt_render_path_passes(pt_scene* scene, const pt_render_desc* desc, const pt_path_passes_desc* passes, float* film_xyzw, float* pass_films, pt_profile* profile);

/* ---- Path expressions: films for user-written light-path patterns ("Path expressions").  An expression describes a path from the camera
 * to an emitter in the event vocabulary of the path passes above:
 *
 *   C              the camera; every alternative starts with it
 *   D R T  .       a diffuse, a reflection, a transmission scattering event (light-tagged vertices scatter too); any of the three
 *   [DR] [^T]      a class of events
 *   ( ) | * + ?    grouping, alternation, repetition over events
 *   L  L0..L7      the terminal "a surface emitter" / "a surface emitter of that light group"
 *   E  E0..E7      the terminal "the environment" / "the environment, if it belongs to that group"
 *   [L2E2]         a class of terminals
 *   CD+L|CR+E      a top-level | joins complete alternatives; every alternative ends in exactly one terminal.  White space is ignored.
 *
 * Expression e's film is the sum over exactly the paths e matches, made from their energies as pt_render's film is made from all of them, whatever other
 * expressions are compiled beside it: expressions may overlap.  The eight path passes are CL, CE, CD[LE], CD.+[LE], CR[LE], CR.+[LE], CT[LE], CT.+[LE]; light
 * group g is C.*[LgEg]; C.*[LE] is the film.
 *
 * The program is the union of the expressions' automata, determinised over the three event symbols (and minimised).  16 bytes per state:
 *   word 0       the successors: bits 0..5 behind D, bits 6..11 behind R, bits 12..17 behind T
 *   words 1..3   nine 8-bit output masks, one per terminal symbol: symbol s in byte s % 4 of word 1 + s / 4.  Symbols 0..7: a surface emitter of group g;
 *                symbol 8: the environment.  Bit e of a mask: expression e accepts a path that ends with this terminal here.
 * E<g> with g != environment_group contributes no bit; L without a digit sets its bit in all eight surface-emitter symbols.  A state from which nothing is
 * accepted is an ordinary state with zero masks.  `start` is the state behind C: the state in front of the camera ray's first vertex.
 * The expression films are left as the scene's resident group films with group_count = outputs, as pass films are.
 * Out of scope: a device mask, spectral bins per expression, hero wavelengths, the medium-aware walk, per-vertex object or material labels. */
#define PT_PATH_EXPRS_MAX 8
#define PT_PATH_EXPR_STATES_MAX 64
#define PT_PATH_EXPR_TERMINALS 9
#define PT_PATH_EXPR_ENVIRONMENT 8    /* the terminal symbol of the environment */

typedef struct pt_path_expr_program {
    uint32_t outputs;                 /* K: 1 .. PT_PATH_EXPRS_MAX */
    uint32_t states;                  /* 1 .. PT_PATH_EXPR_STATES_MAX */
    uint32_t start;                   /* < states */
    uint32_t environment_group;       /* < PT_LIGHT_GROUPS_MAX */
    uint32_t table[PT_PATH_EXPR_STATES_MAX][4];   /* the states' entries; those from `states` on are 0 */
} pt_path_expr_program;

/* Host only.  exprs: n expressions, 1 <= n <= PT_PATH_EXPRS_MAX, expression e tagged with bit e.  err (may be NULL): err_len bytes for the message of a
 * failure, always terminated.  A syntax error is PT_ERR_INVALID_ARGUMENT, reported as "expression <e>, column <c>: ..." with c counted from 1 in the text as
 * given; more than PT_PATH_EXPR_STATES_MAX states is PT_ERR_UNSUPPORTED with a message that names the count. */
pt_status
pt_path_expr_compile(const char* const* exprs, uint32_t n, uint32_t environment_group, pt_path_expr_program* program, char* err, size_t err_len);

/* Host only.  Runs the program over a written-out path — C, events of D R T, one terminal L<g> (L alone: L0) or E — and gives the output mask: bit e set where
 * expression e matches the path.  A malformed path or program is PT_ERR_INVALID_ARGUMENT. */
pt_status
pt_path_expr_match(const pt_path_expr_program* program, const char* path, uint32_t* mask);

/* pt_render_path_passes with the program's expressions where the eight classes stand.  instance_group: one light group id < PT_LIGHT_GROUPS_MAX per instance,
 * n_instances the scene's count; or NULL with n_instances 0: every instance is in group 0.  expr_films: outputs*width*height*4 f32 in the layout of group
 * films, or NULL.  Refused is what pt_render_path_passes refuses, and a malformed program: outputs outside 1..8, states outside 1..64, a successor or the start
 * not below states, a mask bit not below outputs (PT_ERR_INVALID_ARGUMENT). */
pt_status
pt_render_path_exprs(pt_scene* scene, const pt_render_desc* desc, const pt_path_expr_program* program, const uint8_t* instance_group, uint32_t n_instances,
                     float* film_xyzw, float* expr_films, pt_profile* profile);

#ifdef __cplusplus
}
#endif
#endif
