// ptcli — the reference's command line (src/bin/main.rs:30-199) on top of libptscene.so (TOML front end) and libptamd.so
// (HIP engine): read the config, build the scene, render every [[render_settings]] entry on the GPU, write
// output/<filename>.exr and .png through the film output stage (src/renderer/mod.rs:24-80).
//
//   ptcli [--config data/config.toml] [--scene FILE] [-n|--dry-run] [--stdout-log-level L] [--write-log-level L]
//         [--root DIR] [--output-dir DIR] [--seed N] [--write-film] [--adaptive REL] [--devices MASK] [--denoise] [--guide-samples K] [--demodulate-albedo]
//         [--guide-chain D] [--guide-alpha-max A] [--spectral-bins B] [--denoise-spectral-bins B] [--demodulate-bins]
//         [--denoise-light-groups instance|material]
//         [--develop cie|CX,CY,CZ] [--develop-filter CURVE] [--develop-subsamples N] [--spectral-devices MASK] [--denoise-resident]
//         [--denoise-assemble] [--light-groups instance|material] [--light-gains G0,G1,...]
//         [--light-group-devices MASK] [--mattes instance|material] [--matte-ranks R] [--matte-samples S]
//         [--relamp-groups instance|material --relamp-bins B [--relamp G:CURVE[,G:CURVE...]] [--relamp-gains g0,g1,...] [--develop-subsamples N]]
//         [--path-passes] [--denoise-path-passes]
//         [--path-exprs NAME=EXPR;...] [--path-expr-groups instance|material]
//
// --config / --scene / --dry-run / the two log-level options are the reference's (the log levels only select how much
// this program prints: warnings are shown from "warn" up).  --root is where relative file names inside the TOML files
// are looked up when they are not found from the working directory; --write-film also stores the raw XYZ film as
// <filename>.npy for tools/compare_films.py.  --adaptive REL renders every setting that has max_samples > min_samples with
// pt_render_adaptive (include/pt_adaptive.h): min_samples to max_samples per pixel, relative error target REL.  --devices MASK renders every setting on
// the devices of MASK (bit d = HIP device d, 0 = all) from one call: pt_render_multi, or pt_render_adaptive_multi with --adaptive.
// --denoise also writes <filename>_denoised.exr / .png (and .npy with --write-film): the film through pt_denoise_film (include/pt_denoise.h) with guides of
// --guide-samples K camera samples (default 4).  The filter needs the per-pixel statistics, which the adaptive path alone returns: every setting is rendered
// through pt_render_adaptive (max_samples = min_samples without --adaptive: the same film, bit for bit, as pt_render's), and a setting that path refuses — the
// Naive renderer, min_samples not a multiple of 10 — ends the program before anything is rendered.  The files written without the flag stay what they are.
// --demodulate-albedo (with --denoise only) filters the film divided by the first-hit albedo: pt_render_guides_albedo and pt_denoise_film_albedo write the same
// <filename>_denoised.* files.  --guide-chain D (with --denoise only) takes the guides, and the albedo, at the end of every sample's specular chain of at most D
// vertices (pt_render_guides_chain; --guide-alpha-max A: the GGX alpha up to which a material counts as specular, default 0.01).
// --spectral-bins B (1..64) renders every setting through pt_render_spectral (include/pt_spectral.h) and also writes <filename>_spectral.exr: one FLOAT channel
// per wavelength bin (times the factor of the EXR payload) beside the R, G, B of <filename>.exr.  The usual files stay byte for byte what they are.  It is
// refused together with --adaptive, --denoise and a --devices mask that names more than one GPU (or one other than device 0, where the call renders).
// --denoise-spectral-bins B (1..64, with --denoise only) renders every setting through pt_render_adaptive_spectral and filters the film and its bins together
// (pt_denoise_spectral): next to the usual and the _denoised files, which stay byte for byte what --denoise alone writes, it writes <filename>_spectral.exr and
// <filename>_denoised_spectral.exr, the bins times the factor of the EXR payload beside the R, G, B of the film and of the denoised film.  It is refused with
// --spectral-bins, with --demodulate-albedo (the bins have no albedo) and with a --devices mask other than device 0 (the node calls have no spectral film).
// --demodulate-bins (with --denoise-spectral-bins only) takes the guides, the albedo and a per-bin albedo from pt_render_guides_bin_albedo (honouring --guide-chain)
// and filters through pt_denoise_spectral_albedo: the same file names; <filename>_denoised.* become what --denoise --demodulate-albedo writes, byte for byte,
// <filename>_spectral.exr is unchanged and <filename>_denoised_spectral.exr holds the bins of the demodulated filter.
// --develop cie | CX,CY,CZ (with --spectral-bins or --denoise-spectral-bins only) develops the spectral film into a picture: the bins projected onto three response
// curves (pt_spectral_response_matrix, pt_spectral_project*), packed as an XYZW film with W = 0 and sent through the setting's own film output to
// <filename>_developed.exr / .png.  `cie` is the engine's colour-matching fit; CX,CY,CZ are three names of the scene file's curves library (a camera's sensitivities,
// say: they need not be used by the scene).  --develop-filter CURVE multiplies every response by a curve of that library, --develop-subsamples N (1..16, default 1)
// integrates the responses over each bin with N samples.  With --spectral-bins the bins are developed where the render left them on the device
// (pt_spectral_project_resident); with --denoise-spectral-bins the undenoised bins go through pt_spectral_project, and the denoised ones too, to
// <filename>_denoised_developed.*.  Every other file stays byte for byte what it is.  An unknown curve name ends the program once the scene file is loaded.
// --denoise-resident (with --denoise only) runs the guides, the filter and, with --develop, both developments on what the render left on the device
// (include/pt_resident.h: pt_resident_guides, pt_denoise_resident, pt_spectral_project_resident and pt_spectral_project_resident_denoised): the film and the
// bins are not uploaded again.  Every file stays byte for byte what the run without it writes.  It is refused together with --devices and --spectral-devices:
// a node render leaves no film one device can filter.
// --spectral-devices MASK (with --spectral-bins or --denoise-spectral-bins only; bit d = HIP device d, 0 = all) renders the spectral film on the devices of MASK from
// one call: pt_render_spectral_multi, or pt_render_adaptive_spectral_multi with --denoise-spectral-bins.  Every file stays byte for byte what the run without it writes.
// --develop then develops the undenoised bins where the node render left them, shard by shard on the devices (pt_spectral_project_resident), and the filter of
// --denoise runs on the first device of MASK.  It is refused together with --devices, whose refusals of the spectral flags stay what they are.
// --denoise-assemble (with --denoise --denoise-spectral-bins B --spectral-devices MASK only) assembles the node render on the scene's device, device to device
// (pt_resident_assemble: the film from the first device of MASK, every device's packed shard of the bins unpacked into full planes), and runs the guides, the
// filter and, with --develop, the denoised development on the assembled set, as --denoise-resident does after a one-device render: the bins are not uploaded
// again.  The undenoised bins are developed shard by shard where the node render left them, as without the flag.  Every file stays byte for byte what the run
// without it writes.  It is refused together with --denoise-resident, which is the one-device form.
// --light-groups instance|material renders every setting through pt_render_light_groups (include/pt_light_groups.h) and also writes <filename>_light<g>.exr, group g's
// film through the setting's own film output.  `instance`: every emitting instance (a light material as its override, or on a face of its mesh) is a group of its
// own, in scene order; `material`: every light material is, in the order the instances first use them; the environment is the last group when it emits (strength
// other than 0).  What does not emit is in group 0.  More than 8 groups end the program once the scene file is loaded.  The usual files stay byte for byte what they
// are: the film is the total.  --light-gains G0,G1,... (with --light-groups only, one gain per group) also writes <filename>_relit.exr / .png: the group films
// times their gains, mixed where the render left them on the device (pt_light_groups_mix_resident).  Refused together with --adaptive, --denoise, --spectral-bins,
// --denoise-spectral-bins, --devices, --spectral-devices and --hero-wavelengths.
// --relamp-groups instance|material --relamp-bins B renders every setting through pt_render_light_groups_spectral (include/pt_light_groups_spectral.h; groups formed as
// --light-groups forms them) and also writes <filename>_light<g>_spectral.exr, group g's B wavelength bins (pt_write_exr_spectral, in the units of the EXR payload), and
// <filename>_relamped.exr / .png: the colour-matching development of the re-lamped group bins, made where the render left them on the device
// (pt_light_groups_relamp_matrix, pt_light_groups_relamp_resident) and sent through the setting's own film output.  --relamp G:CURVE[,G:CURVE...] shows group G under
// CURVE, a name of the scene file's curves library, in the place of the emission curve its emitters share; --relamp-gains g0,g1,... scales the groups (one gain per
// group); --develop-subsamples N integrates over each bin with N samples.  Without --relamp and --relamp-gains the re-lamped picture is the development of the render
// as it is.  A re-lamped group whose emitters do not share one emission curve, and a re-lamped environment lit by an HDR texture, end the program before anything is
// rendered.  Every usual file stays byte for byte what it is.  Refused together with --adaptive, --denoise, --light-groups, --spectral-bins, --denoise-spectral-bins,
// --devices, --spectral-devices and --hero-wavelengths.
// --denoise-light-groups instance|material (with --denoise only; groups formed as --light-groups forms them) renders every setting through
// pt_render_adaptive_light_groups (include/pt_light_groups_denoise.h) and filters the film and its group films together where the render left them
// (pt_resident_guides, pt_denoise_light_groups_resident), honouring --demodulate-albedo, --guide-chain and --guide-samples; --denoise-resident is accepted and
// changes no file.  The usual files and <filename>_denoised.* are byte for byte those of --denoise with the same other flags; it also writes
// <filename>_light<g>.exr and <filename>_denoised_light<g>.exr and, with --light-gains, <filename>_relit.* and <filename>_denoised_relit.*, the relights of the
// noisy and of the denoised group films (pt_light_groups_mix_resident, pt_light_groups_mix_resident_denoised).  Refused together with --light-groups,
// --spectral-bins, --denoise-spectral-bins, --devices, --spectral-devices, --denoise-assemble and --hero-wavelengths.
// --light-group-devices MASK (with --light-groups or --denoise-light-groups only; bit d = HIP device d, 0 = all) renders the group render on the devices of MASK from
// one call (include/pt_light_groups_multi.h): pt_render_light_groups_multi, or pt_render_adaptive_light_groups_multi with --denoise-light-groups.  Every file stays byte
// for byte what the run without it writes.  The group films are relit where the node render left them, shard by shard on the devices (pt_light_groups_mix_resident).
// With --denoise-light-groups the guides and the joint filter run over host arrays on the first device of MASK (pt_render_guides*, pt_denoise_light_groups) and the
// denoised relight is pt_light_groups_mix of the filtered films; with --denoise-assemble, which this flag allows beside --denoise-light-groups, the node render is
// assembled on the scene's device (pt_resident_assemble: the film, and every device's packed group films unpacked beside it) and guides, filter and denoised relight
// take the resident route of the one-device run.  It is refused together with --devices, whose refusals of the two group flags stay what they are.
// --mattes instance|material also writes <filename>_crypto.exr: the ID mattes of the setting's frame (pt_render_mattes of include/pt_denoise.h; --matte-samples S
// camera samples per pixel, by default the setting's min_samples; --matte-ranks R ranks, by default 6) in the Cryptomatte layout (pt_write_exr_cryptomatte) under
// the layer CryptoObject, instances named instance<i>, or CryptoMaterial, materials named as the scene file's library names them, with the setting's linear RGB
// beside the ranks.  The matte is rendered beside the film: every usual file stays byte for byte what it is.  Refused together with --devices,
// --spectral-devices and --light-group-devices: there is no matte render over a device mask.
// --path-passes renders every setting through pt_render_path_passes (include/pt_light_groups.h, "Path passes") and also writes <filename>_pass_<class>.exr for the
// eight classes — emission, background, diffuse_direct, diffuse_indirect, reflection_direct, reflection_indirect, transmission_direct, transmission_indirect — each
// through the setting's own film output.  The usual files stay byte for byte what they are: the film is the total.  With --denoise --denoise-path-passes every
// setting goes through pt_render_adaptive_path_passes (include/pt_light_groups_denoise.h) and the film and its pass films are filtered together where the render
// left them (pt_resident_guides, pt_denoise_light_groups_resident: the pass films are the scene's resident group films), honouring --adaptive,
// --demodulate-albedo, --guide-chain and --guide-samples; it also writes <filename>_denoised_pass_<class>.exr, and the usual and the _denoised files are byte for
// byte those of --denoise with the same other flags.  Refused with what --light-groups is refused with (--adaptive and --denoise unless --denoise-path-passes is
// given, --spectral-bins, --denoise-spectral-bins, --devices, --spectral-devices, --hero-wavelengths) and with --light-groups, --denoise-light-groups,
// --relamp-groups and --light-group-devices, which use the same resident group films.
// --path-exprs "NAME=EXPR;NAME=EXPR" (up to 8) renders every setting through pt_render_path_exprs (include/pt_light_groups.h, "Path expressions") and also writes
// <filename>_expr_<NAME>.exr, the film of exactly the light paths EXPR matches — caustics=CD[RT]+L, say — through the setting's own film output.  The usual files
// stay byte for byte what they are.  --path-expr-groups instance|material forms light groups as --light-groups forms them, for the terminals L0..L7 and E0..E7;
// without it every emitter is in group 0, the environment too.  An expression outside the language ends the program with the compiler's message before any
// file is read.  Refused with what --path-passes is refused with, with --path-passes itself and with --denoise.
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/pt_adaptive.h"
#include "../../../include/pt_denoise.h"
#include "../../../include/pt_light_groups.h"
#include "../../../include/pt_light_groups_denoise.h"
#include "../../../include/pt_light_groups_multi.h"
#include "../../../include/pt_light_groups_spectral.h"
#include "../../../include/pt_scene_file.h"
#include "../../../include/pt_resident.h"
#include "../../../include/pt_spectral.h"

namespace {

struct Options {
    std::string config = "data/config.toml", scene, root, output_dir = "output", stdout_log_level = "warn";
    bool has_scene = false, dry_run = false, write_film = false;
    uint32_t hero = 0;   // --hero-wavelengths: 0 = as the render settings say (1)
    uint64_t seed = 1;
    float adaptive = -1.0f;   // --adaptive REL: the relative error target; < 0 = off
    bool multi = false;       // --devices MASK: the node calls (pt_render_multi / pt_render_adaptive_multi)
    uint64_t device_mask = 0;
    bool denoise = false;     // --denoise: <filename>_denoised.* next to the outputs
    uint32_t guide_samples = 4;
    bool demodulate = false;  // --demodulate-albedo: the denoised files through the albedo entries
    bool chain = false;       // --guide-chain D: the guides through pt_render_guides_chain
    uint32_t max_chain = 0;
    float alpha_max = 0.0f;   // --guide-alpha-max A (0 = the default)
    bool has_alpha_max = false;
    uint32_t spectral_bins = 0;   // --spectral-bins B: <filename>_spectral.exr through pt_render_spectral; 0 = off
    uint32_t denoise_bins = 0;    // --denoise-spectral-bins B: the adaptive spectral render and the joint filter; 0 = off
    bool demodulate_bins = false; // --demodulate-bins: the joint filter through the per-bin albedo entries
    bool develop = false;         // --develop: <filename>_developed.* from the bins
    std::vector<std::string> develop_curves;   // three names of the curves library; empty = the colour-matching fit
    bool has_develop_filter = false, has_develop_subsamples = false;
    std::string develop_filter;
    uint32_t develop_subsamples = 1;
    bool resident = false;        // --denoise-resident: guides, filter and developments on the scene's resident set (include/pt_resident.h)
    bool spectral_multi = false;  // --spectral-devices MASK: the spectral node calls (pt_render_spectral_multi / pt_render_adaptive_spectral_multi)
    uint64_t spectral_device_mask = 0;
    int light_groups = 0;         // --light-groups: 1 = a group per emitting instance, 2 = per light material; 0 = off
    bool has_light_gains = false; // --light-gains: <filename>_relit.* from the resident mix
    int denoise_groups = 0;       // --denoise-light-groups: the adaptive group render and the joint filter over the group films; 1 | 2 as light_groups, 0 = off
    std::vector<float> light_gains;
    int relamp_groups = 0;        // --relamp-groups: the spectral group render and the re-lamped picture; 1 | 2 as light_groups, 0 = off
    uint32_t relamp_bins = 0;     // --relamp-bins B
    bool has_relamp = false, has_relamp_gains = false;
    std::vector<std::pair<uint32_t, std::string>> relamp;   // --relamp G:CURVE,...
    std::vector<float> relamp_gains;                        // --relamp-gains
    bool group_multi = false;     // --light-group-devices MASK: the group node calls (pt_render_light_groups_multi / pt_render_adaptive_light_groups_multi)
    uint64_t group_device_mask = 0;
    bool assemble = false;        // --denoise-assemble: the node render assembled on the scene's device, then as `resident` (pt_resident_assemble)
    int mattes = 0;               // --mattes: <filename>_crypto.exr through pt_render_mattes; 1 = keyed by instance, 2 = by material; 0 = off
    uint32_t matte_ranks = 6, matte_samples = 0;   // --matte-ranks R, --matte-samples S (0 = the setting's min_samples)
    bool has_matte_ranks = false, has_matte_samples = false;
    bool path_passes = false;     // --path-passes: <filename>_pass_<class>.exr through pt_render_path_passes
    bool denoise_passes = false;  // --denoise-path-passes: the adaptive pass render and the joint filter over the pass films
    std::vector<std::pair<std::string, std::string>> path_exprs;   // --path-exprs: (NAME, EXPR), <filename>_expr_<NAME>.exr through pt_render_path_exprs; empty = off
    int expr_groups = 0;          // --path-expr-groups: the light groups of the expressions' terminals; 1 | 2 as light_groups, 0 = every emitter in group 0
};

const char* const kPathPassNames[PT_PATH_PASSES] = {"emission", "background", "diffuse_direct", "diffuse_indirect", "reflection_direct", "reflection_indirect",
                                                    "transmission_direct", "transmission_indirect"};

int usage(const std::string& msg) {   // ("": the usage alone)
    if (!msg.empty()) fprintf(stderr, "error: %s\n", msg.c_str());
    fprintf(stderr, "usage: ptcli [--config FILE] [--scene FILE] [-n|--dry-run] [--stdout-log-level LEVEL] [--write-log-level LEVEL]\n"
                    "             [--root DIR] [--output-dir DIR] [--seed N] [--write-film] [--hero-wavelengths 1|4] [--adaptive REL] [--devices MASK]\n"
                    "             [--denoise] [--guide-samples K] [--demodulate-albedo] [--guide-chain D] [--guide-alpha-max A]\n"
                    "             [--spectral-bins B] [--denoise-spectral-bins B] [--demodulate-bins]\n"
                    "             [--denoise-light-groups instance|material]\n"
                    "             [--develop cie|CX,CY,CZ] [--develop-filter CURVE] [--develop-subsamples N] [--spectral-devices MASK]\n"
                    "             [--denoise-resident] [--denoise-assemble] [--light-groups instance|material] [--light-gains G0,G1,...]\n"
                    "             [--light-group-devices MASK] [--mattes instance|material] [--matte-ranks R] [--matte-samples S]\n"
                    "             [--relamp-groups instance|material --relamp-bins B [--relamp G:CURVE[,G:CURVE...]] [--relamp-gains g0,g1,...]\n"
                    "              [--develop-subsamples N]]\n"
                    "             [--path-passes] [--denoise-path-passes]\n"
                    "             [--path-exprs NAME=EXPR;...] [--path-expr-groups instance|material]\n");
    return 2;
}

bool write_npy(const std::string& path, const float* data, uint32_t h, uint32_t w) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(h) + ", " + std::to_string(w) + ", 4), }";
    while ((10 + dict.size() + 1) % 64) dict += ' ';
    dict += '\n';
    uint8_t head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (uint8_t)(dict.size() & 255), (uint8_t)(dict.size() >> 8)};
    bool ok = fwrite(head, 1, 10, f) == 10 && fwrite(dict.data(), 1, dict.size(), f) == dict.size() &&
              fwrite(data, sizeof(float), (size_t)w * h * 4, f) == (size_t)w * h * 4;
    fclose(f);
    return ok;
}

// ---- the value parsers: a flag's arm of the option loop calls these and keeps its own field, has_* flag and message

bool parse_count(const std::string& v, unsigned long lo, unsigned long hi, uint32_t* out) {   // a decimal count in [lo, hi], the whole string
    char* end = nullptr;
    const unsigned long x = strtoul(v.c_str(), &end, 10);
    if (end == v.c_str() || *end || x < lo || x > hi) return false;
    *out = (uint32_t)x;
    return true;
}

bool parse_mask(const std::string& v, uint64_t* out) {   // a device mask in any base of strtoull, the whole string
    char* end = nullptr;
    *out = strtoull(v.c_str(), &end, 0);
    return end != v.c_str() && !*end;
}

bool parse_float(const std::string& v, float* out) {   // the whole string (the caller checks the range)
    char* end = nullptr;
    *out = strtof(v.c_str(), &end);
    return end != v.c_str() && !*end;
}

int parse_group_mode(const std::string& v) { return v == "instance" ? 1 : v == "material" ? 2 : 0; }

std::vector<std::string> split(const std::string& v) {   // at every comma: "" is one empty item
    std::vector<std::string> items;
    for (size_t p = 0;;) {
        const size_t c = v.find(',', p);
        items.push_back(v.substr(p, c == std::string::npos ? std::string::npos : c - p));
        if (c == std::string::npos) return items;
        p = c + 1;
    }
}

// a list of gains: 0 = taken, 1 = an item is no finite float (|g| < 1e30), 2 = more than PT_LIGHT_GROUPS_MAX of them
int parse_gains(const std::string& v, std::vector<float>* out) {
    out->clear();
    for (const std::string& item : split(v)) {
        float g = 0.0f;
        if (!parse_float(item, &g) || !(g > -1e30f && g < 1e30f)) return 1;
        out->push_back(g);
    }
    return out->size() > PT_LIGHT_GROUPS_MAX ? 2 : 0;
}

std::string trimmed(const std::string& v) {
    const size_t a = v.find_first_not_of(" \t"), b = v.find_last_not_of(" \t");
    return a == std::string::npos ? "" : v.substr(a, b - a + 1);
}

// the expressions of a set in the order given, compiled for an environment in `environment_group`: "" or the compiler's message
std::string compile_path_exprs(const std::vector<std::pair<std::string, std::string>>& exprs, uint32_t environment_group, pt_path_expr_program* program) {
    std::vector<const char*> texts;
    for (const auto& e : exprs) texts.push_back(e.second.c_str());
    char err[512];
    return pt_path_expr_compile(texts.data(), (uint32_t)texts.size(), environment_group, program, err, sizeof(err)) == PT_OK ? "" : err;
}

// --path-exprs NAME=EXPR;NAME=EXPR: "" when taken, else the message.  A name goes into a file name: letters, digits, '_', '-' and '.'.
std::string parse_path_exprs(const std::string& v, std::vector<std::pair<std::string, std::string>>* out) {
    out->clear();
    for (size_t p = 0;;) {
        const size_t c = v.find(';', p);
        const std::string item = v.substr(p, c == std::string::npos ? std::string::npos : c - p);
        const size_t eq = item.find('=');
        const std::string name = trimmed(item.substr(0, eq)), expr = eq == std::string::npos ? "" : trimmed(item.substr(eq + 1));
        if (eq == std::string::npos || name.empty() || expr.empty()) return "--path-exprs takes NAME=EXPR;NAME=EXPR";
        for (char ch : name)
            if (!((ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '-' || ch == '.'))
                return "--path-exprs: the name '" + name + "' goes into a file name: letters, digits, '_', '-' and '.' only";
        for (const auto& have : *out) if (have.first == name) return "--path-exprs names '" + name + "' twice";
        out->push_back({name, expr});
        if (c == std::string::npos) break;
        p = c + 1;
    }
    if (out->size() > PT_PATH_EXPRS_MAX) return "--path-exprs takes at most 8 expressions";
    pt_path_expr_program program;   // (the syntax, before any file is read; the program itself is compiled once the environment's group is known)
    const std::string mistake = compile_path_exprs(*out, 0u, &program);
    return mistake.empty() ? "" : "--path-exprs: " + mistake;
}

// the flags that take a value: the option loop fetches it, or refuses the flag without one, before the flag's arm runs
const char* const kValueFlags[] = {"--config", "--scene", "--stdout-log-level", "--write-log-level", "--root", "--output-dir", "--seed", "--hero-wavelengths",
                                   "--adaptive", "--devices", "--guide-samples", "--guide-chain", "--guide-alpha-max", "--spectral-bins", "--denoise-spectral-bins",
                                   "--develop", "--develop-filter", "--develop-subsamples", "--spectral-devices", "--light-group-devices", "--light-groups",
                                   "--relamp-groups", "--relamp-bins", "--relamp", "--relamp-gains", "--denoise-light-groups", "--light-gains", "--mattes",
                                   "--matte-ranks", "--matte-samples", "--path-exprs", "--path-expr-groups"};

// The option loop: "" when the command line parsed, else the message for usage().  *help: -h was met before any mistake.
std::string parse_options(int argc, char** argv, Options& o, bool* help) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        std::string v;
        bool takes_value = false;
        for (const char* flag : kValueFlags) takes_value = takes_value || a == flag;
        if (takes_value) {
            if (i + 1 >= argc) return a == "--develop-filter" ? "--develop-filter needs a curve name" : a + " needs a value";
            v = argv[++i];
        }
        if (a == "--config") o.config = v;
        else if (a == "--scene") { o.scene = v; o.has_scene = true; }
        else if (a == "-n" || a == "--dry-run") o.dry_run = true;
        else if (a == "--stdout-log-level") o.stdout_log_level = v;
        else if (a == "--write-log-level") {}   // (nothing is written to a log file)
        else if (a == "--root") o.root = v;
        else if (a == "--output-dir") o.output_dir = v;
        else if (a == "--seed") o.seed = strtoull(v.c_str(), nullptr, 10);
        else if (a == "--write-film") o.write_film = true;
        else if (a == "--hero-wavelengths") o.hero = (uint32_t)strtoul(v.c_str(), nullptr, 10);
        else if (a == "--adaptive") { if (!parse_float(v, &o.adaptive) || !(o.adaptive >= 0.0f)) return "--adaptive needs a relative error >= 0"; }
        else if (a == "--devices") { if (!parse_mask(v, &o.device_mask)) return "--devices needs a device mask (bit d = HIP device d, 0 = all)"; o.multi = true; }
        else if (a == "--denoise") o.denoise = true;
        else if (a == "--demodulate-albedo") o.demodulate = true;
        else if (a == "--demodulate-bins") o.demodulate_bins = true;
        else if (a == "--denoise-resident") o.resident = true;
        else if (a == "--denoise-assemble") o.assemble = true;
        // (these two take any count that strtoul reads and look at what is left of it in 32 bits)
        else if (a == "--guide-samples") { if (!parse_count(v, 0, ~0ul, &o.guide_samples) || o.guide_samples == 0) return "--guide-samples needs a positive count"; }
        else if (a == "--guide-chain") { if (!parse_count(v, 0, ~0ul, &o.max_chain) || o.max_chain > PT_GUIDE_CHAIN_MAX) return "--guide-chain needs a count of at most 16"; o.chain = true; }
        else if (a == "--guide-alpha-max") { if (!parse_float(v, &o.alpha_max) || !(o.alpha_max >= 0.0f) || !(o.alpha_max < 1e30f)) return "--guide-alpha-max needs a finite alpha >= 0"; o.has_alpha_max = true; }
        else if (a == "--spectral-bins") { if (!parse_count(v, 1, PT_SPECTRAL_MAX_BINS, &o.spectral_bins)) return "--spectral-bins needs a count in 1..64"; }
        else if (a == "--denoise-spectral-bins") { if (!parse_count(v, 1, PT_SPECTRAL_MAX_BINS, &o.denoise_bins)) return "--denoise-spectral-bins needs a count in 1..64"; }
        else if (a == "--develop") {
            o.develop_curves.clear();
            if (v != "cie") {
                o.develop_curves = split(v);
                bool ok = o.develop_curves.size() == 3;
                for (const std::string& n : o.develop_curves) ok = ok && !n.empty();
                if (!ok) return "--develop needs `cie` or three curve names CX,CY,CZ";
            }
            o.develop = true;
        }
        else if (a == "--develop-filter") { if (v.empty()) return "--develop-filter needs a curve name"; o.develop_filter = v; o.has_develop_filter = true; }
        else if (a == "--develop-subsamples") { if (!parse_count(v, 1, PT_SPECTRAL_MAX_SUBSAMPLES, &o.develop_subsamples)) return "--develop-subsamples needs a count in 1..16"; o.has_develop_subsamples = true; }
        else if (a == "--spectral-devices") { if (!parse_mask(v, &o.spectral_device_mask)) return "--spectral-devices needs a device mask (bit d = HIP device d, 0 = all)"; o.spectral_multi = true; }
        else if (a == "--light-group-devices") { if (!parse_mask(v, &o.group_device_mask)) return "--light-group-devices needs a device mask (bit d = HIP device d, 0 = all)"; o.group_multi = true; }
        else if (a == "--light-groups") { if (!(o.light_groups = parse_group_mode(v))) return "--light-groups needs `instance` or `material`"; }
        else if (a == "--relamp-groups") { if (!(o.relamp_groups = parse_group_mode(v))) return "--relamp-groups needs `instance` or `material`"; }
        else if (a == "--relamp-bins") { if (!parse_count(v, 1, PT_SPECTRAL_MAX_BINS, &o.relamp_bins)) return "--relamp-bins needs a count in 1..64"; }
        else if (a == "--relamp") {
            o.has_relamp = true;
            o.relamp.clear();
            for (const std::string& item : split(v)) {
                const size_t colon = item.find(':');
                uint32_t g = 0;
                if (colon == std::string::npos || !parse_count(item.substr(0, colon), 0, PT_LIGHT_GROUPS_MAX - 1, &g) || colon + 1 >= item.size())
                    return "--relamp needs G:CURVE[,G:CURVE...] with G a group in 0..7";
                for (const auto& have : o.relamp) if (have.first == g) return "--relamp names a group twice";
                o.relamp.push_back({g, item.substr(colon + 1)});
            }
        }
        else if (a == "--relamp-gains") { o.has_relamp_gains = true; if (const int bad = parse_gains(v, &o.relamp_gains)) return bad == 1 ? "--relamp-gains needs finite gains g0,g1,..." : "--relamp-gains takes at most 8 gains"; }
        else if (a == "--denoise-light-groups") { if (!(o.denoise_groups = parse_group_mode(v))) return "--denoise-light-groups needs `instance` or `material`"; }
        else if (a == "--light-gains") { o.has_light_gains = true; if (const int bad = parse_gains(v, &o.light_gains)) return bad == 1 ? "--light-gains needs finite gains G0,G1,..." : "--light-gains takes at most 8 gains"; }
        else if (a == "--mattes") { if (!(o.mattes = parse_group_mode(v))) return "--mattes needs `instance` or `material`"; }
        else if (a == "--matte-ranks") { if (!parse_count(v, 1, PT_MATTE_RANKS_MAX, &o.matte_ranks)) return "--matte-ranks needs a number of ranks in 1..8"; o.has_matte_ranks = true; }
        else if (a == "--matte-samples") { if (!parse_count(v, 1, 65535, &o.matte_samples)) return "--matte-samples needs a number of samples in 1..65535"; o.has_matte_samples = true; }
        else if (a == "--path-passes") o.path_passes = true;
        else if (a == "--denoise-path-passes") o.denoise_passes = true;
        else if (a == "--path-exprs") { const std::string mistake = parse_path_exprs(v, &o.path_exprs); if (!mistake.empty()) return mistake; }
        else if (a == "--path-expr-groups") { if (!(o.expr_groups = parse_group_mode(v))) return "--path-expr-groups needs `instance` or `material`"; }
        else if (a == "-h" || a == "--help") { *help = true; return ""; }
        else return "unknown option " + a;
    }
    return "";
}

// ---- the combination rules: "" when the flags go together, else the message for usage().  The order of the rules, and the order inside each list, decides which
// message a command line that breaks several of them gets.

struct Present { bool present; const char* flag; };

std::string cannot_combine(const char* flag, std::initializer_list<Present> others, const char* why) {   // ("" when none of the others is present)
    for (const Present& other : others) if (other.present) return std::string(flag) + " cannot be combined with " + other.flag + ": " + why;
    return "";
}

std::string check_options(const Options& o) {
    std::string no;
    const bool adaptive = o.adaptive >= 0.0f;
    const Present adapt{adaptive, "--adaptive"}, denoise{o.denoise, "--denoise"}, bins{o.spectral_bins != 0, "--spectral-bins"}, dbins{o.denoise_bins != 0, "--denoise-spectral-bins"},
                  devices{o.multi, "--devices"}, sdevices{o.spectral_multi, "--spectral-devices"}, gdevices{o.group_multi, "--light-group-devices"}, hero{o.hero != 0, "--hero-wavelengths"},
                  groups{o.light_groups != 0, "--light-groups"}, dgroups{o.denoise_groups != 0, "--denoise-light-groups"}, relamp{o.relamp_groups != 0, "--relamp-groups"};
    if (o.denoise_passes && !(o.path_passes && o.denoise)) return "--denoise-path-passes needs --path-passes and --denoise";
    if (o.path_passes) {
        no = cannot_combine("--path-passes", {{adaptive && !o.denoise_passes, "--adaptive"}, bins, dbins, devices, sdevices, hero, groups, dgroups, relamp, gdevices, {o.assemble, "--denoise-assemble"}},
                            "a pass render is one render of one wavelength per path on one device, and its films are the scene's resident group films");
        if (!no.empty()) return no;
        if (o.denoise && !o.denoise_passes) return "--path-passes cannot be combined with --denoise without --denoise-path-passes: the filter of the pass films takes the adaptive pass render";
    }
    if (o.expr_groups && o.path_exprs.empty()) return "--path-expr-groups needs --path-exprs";
    if (!o.path_exprs.empty()) {
        no = cannot_combine("--path-exprs", {adapt, denoise, bins, dbins, devices, sdevices, hero, groups, dgroups, relamp, gdevices, {o.path_passes, "--path-passes"}, {o.assemble, "--denoise-assemble"}},
                            "an expression render is one plain render of one wavelength per path on one device, and its films are the scene's resident group films");
        if (!no.empty()) return no;
    }
    if (o.group_multi && !o.light_groups && !o.denoise_groups) return "--light-group-devices needs --light-groups or --denoise-light-groups: it names the devices their group render runs on";
    if (o.group_multi && o.multi) return "--light-group-devices cannot be combined with --devices: a group render takes its devices from --light-group-devices alone";
    if (o.relamp_groups) {
        no = cannot_combine("--relamp-groups", {adapt, denoise, groups, bins, dbins, devices, sdevices, hero}, "a spectral group render is one plain render of one wavelength per path on one device");
        if (!no.empty()) return no;
        if (!o.relamp_bins) return "--relamp-groups needs --relamp-bins";
    } else {
        if (o.relamp_bins) return "--relamp-bins needs --relamp-groups";
        if (o.has_relamp) return "--relamp needs --relamp-groups";
        if (o.has_relamp_gains) return "--relamp-gains needs --relamp-groups";
    }
    if (o.denoise_groups) {
        no = cannot_combine("--denoise-light-groups", {groups, bins, dbins, devices, sdevices, {o.assemble && !o.group_multi, "--denoise-assemble"}, hero},
                            "it is one adaptive group render of one wavelength per path on one device, and its filter");
        if (!no.empty()) return no;
        if (!o.denoise) return "--denoise-light-groups needs --denoise";
    }
    if (o.has_light_gains && !o.light_groups && !o.denoise_groups) return "--light-gains needs --light-groups";
    if (o.light_groups) {
        no = cannot_combine("--light-groups", {adapt, denoise, bins, dbins, devices, sdevices, hero}, "a group render is one plain render of one wavelength per path on one device");
        if (!no.empty()) return no;
    }
    if (o.mattes) {
        no = cannot_combine("--mattes", {devices, sdevices, gdevices}, "a matte render runs on the scene's device and there is none over a device mask");
        if (!no.empty()) return no;
    } else if (o.has_matte_ranks || o.has_matte_samples) return o.has_matte_ranks ? "--matte-ranks needs --mattes" : "--matte-samples needs --mattes";
    if (o.demodulate && !o.denoise) return "--demodulate-albedo needs --denoise";
    if (o.chain && !o.denoise) return "--guide-chain needs --denoise";
    if (o.has_alpha_max && !o.chain) return "--guide-alpha-max needs --guide-chain";
    if (o.denoise_bins && o.spectral_bins) return "--denoise-spectral-bins cannot be combined with --spectral-bins: it writes the spectral files itself";
    if (o.spectral_bins && adaptive) return "--spectral-bins cannot be combined with --adaptive: an adaptive render has no spectral film";
    if (o.spectral_bins && o.denoise) return "--spectral-bins cannot be combined with --denoise: the denoiser takes the adaptive path, which has no spectral film";
    if (o.spectral_bins && o.multi) {   // (pt_render_spectral renders on the scene's device, device 0: a mask may name that one alone; 0 = every device of the node)
        if ((o.device_mask & (o.device_mask - 1)) != 0 || (o.device_mask == 0 && pt_device_count() > 1))
            return "--spectral-bins cannot be combined with --devices naming more than one GPU: pt_render_multi has no spectral film";
        if (o.device_mask > 1) return "--spectral-bins renders on device 0: --devices may name that device alone";
    }
    if (o.resident && !o.denoise) return "--denoise-resident needs --denoise";
    if (o.resident && o.multi) return "--denoise-resident cannot be combined with --devices: a node render leaves no film one device can filter";
    if (o.resident && o.group_multi) return "--denoise-resident cannot be combined with --light-group-devices: a node render leaves no film one device can filter (--denoise-assemble gathers one)";
    if (o.resident && o.spectral_multi) return "--denoise-resident cannot be combined with --spectral-devices: a node render leaves no film one device can filter";
    if (o.demodulate_bins && !o.denoise_bins) return "--demodulate-bins needs --denoise-spectral-bins";
    if (o.denoise_bins && !o.denoise) return "--denoise-spectral-bins needs --denoise";
    if (o.denoise_bins && o.demodulate) return "--denoise-spectral-bins cannot be combined with --demodulate-albedo: demodulating the bins needs a per-bin albedo";
    if (o.denoise_bins && o.multi && o.device_mask != 1) return "--denoise-spectral-bins renders on device 0: --devices may name that device alone";
    if (o.develop && !o.spectral_bins && !o.denoise_bins) return "--develop needs --spectral-bins or --denoise-spectral-bins: it develops their bins";
    if (o.has_develop_filter && !o.develop) return "--develop-filter needs --develop";
    if (o.has_develop_subsamples && !o.develop && !o.relamp_groups) return "--develop-subsamples needs --develop";
    if (o.spectral_multi && !o.spectral_bins && !o.denoise_bins) return "--spectral-devices needs --spectral-bins or --denoise-spectral-bins: it names the devices their spectral film is rendered on";
    if (o.spectral_multi && o.multi) return "--spectral-devices cannot be combined with --devices: a spectral render takes its devices from --spectral-devices alone";
    if (o.assemble && o.resident) return "--denoise-assemble cannot be combined with --denoise-resident: that flag is the one-device form, this one assembles a node render";
    if (o.assemble && !o.denoise) return "--denoise-assemble needs --denoise";
    const bool assemble_groups = o.assemble && o.denoise_groups && o.group_multi;   // (the node group render assembled: the other form of the flag)
    if (o.assemble && !assemble_groups && !o.denoise_bins) return "--denoise-assemble needs --denoise-spectral-bins: it assembles the node render of the spectral film";
    if (o.assemble && !assemble_groups && !o.spectral_multi) return "--denoise-assemble needs --spectral-devices: it assembles the node render on those devices";
    return "";
}

// ---- what a run holds from loading to the last setting.  The owners free in reverse order: the scene, the scene file, the config.

template <class T, void (*Free)(T*)>
struct Freeing { void operator()(T* p) const { Free(p); } };

bool fail(const char* prefix) {   // the engine's last error under a site's own prefix
    fprintf(stderr, "%s: %s\n", prefix, pt_last_error());
    return false;
}

uint32_t first_device(uint64_t mask) {   // the lowest device of a mask; 0 for the mask 0 (= all devices)
    uint32_t d = 0;
    if (mask) while (!((mask >> d) & 1u)) ++d;
    return d;
}

std::vector<float> pack_planes(const std::vector<float>& planes, size_t np) {   // three planes as an XYZW film with W = 0
    std::vector<float> packed(4 * np);
    for (size_t p = 0; p < np; ++p) { packed[4 * p] = planes[p]; packed[4 * p + 1] = planes[np + p]; packed[4 * p + 2] = planes[2 * np + p]; packed[4 * p + 3] = 0.0f; }
    return packed;
}

// An instance's light materials: its override, else every face material of its mesh.  `visit(id)` returns false to stop the walk.
template <class Visit>
void for_each_light_material(const pt_scene_desc* desc, const pt_instance& in, Visit visit) {
    if (in.material != PT_MATERIAL_NONE) { if (PT_MATERIAL_TAG(in.material) == PT_TAG_LIGHT) visit(in.material); }
    else if (in.kind == PT_SHAPE_MESH && in.mesh >= 0 && (uint32_t)in.mesh < desc->mesh_count && desc->meshes[in.mesh].face_material_offset >= 0) {
        const pt_mesh& m = desc->meshes[in.mesh];
        for (uint32_t f = 0; f < m.face_count; ++f) {
            const uint32_t id = desc->face_materials[(size_t)m.face_material_offset + f];
            if (PT_MATERIAL_TAG(id) == PT_TAG_LIGHT && !visit(id)) return;
        }
    }
}

struct Curves {   // curves in pt_scene_desc's representation, for the response and re-lamp matrices
    std::vector<pt_curve> curves;
    std::vector<float> data;
    // appends a curve of the scene file's library: its index, or -1 (pt_scene_file_last_error says why)
    int32_t add(pt_scene_file* scene_file, const std::string& name) {
        pt_curve c; const float* from = nullptr; uint32_t floats = 0;
        if (pt_scene_file_library_curve(scene_file, name.c_str(), &c, &from, &floats) != PT_OK) return -1;
        c.data_offset = (uint32_t)data.size();
        data.insert(data.end(), from, from + floats);
        curves.push_back(c);
        return (int32_t)curves.size() - 1;
    }
};

struct Run {
    Options o;
    bool warnings = false;
    std::unique_ptr<pt_config, Freeing<pt_config, pt_config_free>> config;
    std::unique_ptr<pt_scene_file, Freeing<pt_scene_file, pt_scene_file_free>> scene_file;
    std::unique_ptr<pt_scene, Freeing<pt_scene, pt_scene_destroy>> scene;
    const pt_scene_desc* desc = nullptr;
    // --develop: the response curves and the filter, from the curves library of the scene file
    Curves develop_curves;
    int32_t develop_responses[3] = {PT_RESPONSE_CIE_X, PT_RESPONSE_CIE_Y, PT_RESPONSE_CIE_Z}, develop_filter = PT_SPECTRAL_NO_FILTER;
    // the three group flags: a group per emitting instance or per light material in scene order, the environment last when it emits
    int group_mode = 0;
    const char* group_flag = "";
    std::vector<uint8_t> instance_group;
    pt_light_groups_desc gd;
    // --relamp-groups: the curves of pt_light_groups_relamp_matrix — the scene's own, where a group's old curve is, and behind them the new ones from the curves
    // library of the scene file — and per group the old and the new curve
    Curves relamp_curves;
    std::vector<int32_t> relamp_old = std::vector<int32_t>(PT_LIGHT_GROUPS_MAX, PT_RELAMP_KEEP), relamp_new = relamp_old;
    // --path-exprs: the program of the expressions, compiled for the environment's group of --path-expr-groups (without that flag: 0, and no instance is labelled)
    pt_path_expr_program expr_program;
};

// The exits between loading the scene and rendering: each says why on stderr and returns false.

bool load_develop_curves(Run& r) {
    std::vector<std::string> names = r.o.develop_curves;
    if (r.o.has_develop_filter) names.push_back(r.o.develop_filter);
    for (size_t k = 0; k < names.size(); ++k) {
        if (r.develop_curves.add(r.scene_file.get(), names[k]) < 0) { fprintf(stderr, "error: --develop: %s\n", pt_scene_file_last_error()); return false; }
        if (k < r.o.develop_curves.size()) r.develop_responses[k] = (int32_t)k; else r.develop_filter = (int32_t)k;
    }
    return true;
}

bool form_light_groups(Run& r) {
    const Options& o = r.o;
    const pt_scene_desc* desc = r.desc;
    std::vector<uint32_t> keys;   // a group's key: the instance (mode 1) or the packed light material (mode 2)
    for (uint32_t i = 0; i < desc->instance_count; ++i) {
        uint32_t light = PT_MATERIAL_NONE;   // the instance's first light material
        for_each_light_material(desc, desc->instances[i], [&](uint32_t id) { light = id; return false; });
        if (light == PT_MATERIAL_NONE) continue;
        const uint32_t key = r.group_mode == 1 ? i : light;
        uint32_t g = 0;
        while (g < keys.size() && keys[g] != key) ++g;
        if (g == keys.size()) keys.push_back(key);
        if (g < PT_LIGHT_GROUPS_MAX) r.instance_group[i] = (uint8_t)g;
    }
    uint32_t groups = (uint32_t)keys.size();
    const bool env_emits = desc->environment.strength != 0.0f;
    r.gd.environment_group = env_emits ? groups : 0u;
    if (env_emits) ++groups;
    if (groups == 0) groups = 1;
    const char* why = groups > PT_LIGHT_GROUPS_MAX ? "the scene has more than 8 light groups"
                      : (o.has_light_gains && o.light_gains.size() != groups) ? "--light-gains needs one gain per group" : nullptr;
    if (why) { fprintf(stderr, "error: %s: %s (%u groups)\n", r.group_flag, why, groups); return false; }
    r.gd.group_count = groups; r.gd.instance_count = desc->instance_count; r.gd.instance_group = r.instance_group.data();
    printf("light groups: %u (%s%s)\n", groups, r.group_mode == 1 ? "one per emitting instance" : "one per light material", env_emits ? ", the environment last" : "");
    return true;
}

bool load_relamp_curves(Run& r) {
    const Options& o = r.o;
    const pt_scene_desc* desc = r.desc;
    const pt_light_groups_desc& gd = r.gd;
    const auto refuse = [](const std::string& why) { fprintf(stderr, "error: --relamp-groups: %s\n", why.c_str()); return false; };
    if (o.has_relamp_gains && o.relamp_gains.size() != gd.group_count) return refuse("--relamp-gains needs one gain per group (" + std::to_string(gd.group_count) + " groups)");
    r.relamp_curves.curves.assign(desc->curves, desc->curves + desc->curve_count);
    r.relamp_curves.data.assign(desc->curve_data, desc->curve_data + desc->curve_data_count);
    const bool env_emits = desc->environment.strength != 0.0f;
    for (const auto& item : o.relamp) {
        const uint32_t g = item.first;
        const std::string names = "--relamp names group " + std::to_string(g);
        if (g >= gd.group_count) return refuse(names + ", the scene has " + std::to_string(gd.group_count) + " groups");
        // the emission curve the group's emitters share: every light material of its instances, and the environment's curve when it is the environment's group
        int32_t old = -1;
        bool mixed = false, any = false;
        const auto emitter = [&](int32_t curve) { mixed = mixed || (any && curve != old); old = curve; any = true; };
        if (env_emits && gd.environment_group == g) {
            if (desc->environment.kind == PT_ENV_HDR) return refuse(names + ", the environment, which an HDR texture lights: it has no single emission curve to replace");
            emitter(desc->environment.curve);
        }
        for (uint32_t i = 0; i < desc->instance_count; ++i) {
            if (r.instance_group[i] != g) continue;
            for_each_light_material(desc, desc->instances[i], [&](uint32_t id) {
                if (PT_MATERIAL_INDEX(id) < desc->material_count) emitter(desc->materials[PT_MATERIAL_INDEX(id)].curve_emit);
                return true;
            });
        }
        if (!any) return refuse(names + ", which holds no emitter");
        if (mixed) return refuse(names + ", whose emitters have different emission curves: it has no single curve to replace");
        const int32_t fresh = r.relamp_curves.add(r.scene_file.get(), item.second);
        if (fresh < 0) return refuse(std::string("--relamp: ") + pt_scene_file_last_error());
        r.relamp_old[g] = old; r.relamp_new[g] = fresh;
    }
    return true;
}

// --denoise: what the adaptive path refuses is refused here, with its message, before anything is rendered or written
bool adaptive_path_takes_every_setting(const Run& r) {
    const Options& o = r.o;
    uint32_t tw = 0, th = 0;
    const bool naive = pt_config_renderer(r.config.get(), &tw, &th) == PT_RENDERER_NAIVE;
    for (uint32_t i = 0; i < pt_config_render_settings_count(r.config.get()); ++i) {
        pt_render_settings rs; pt_render_desc rd;
        pt_config_render_settings(r.config.get(), i, &rs);
        if (pt_config_render_desc(r.config.get(), i, o.seed, &rd) != PT_OK) continue;   // (skipped when rendering as well)
        const bool range = o.adaptive >= 0.0f && !naive && rs.max_samples >= 0 && (uint32_t)rs.max_samples > rd.spp;   // (--adaptive rounds a range up itself)
        const char* why = naive ? "adaptive sampling needs phases of 10 samples (phase_samples 0 or 10)"
                                : ((!range && rd.spp % 10u != 0u) ? "spp, step and max_samples must be multiples of 10" : nullptr);
        if (why) {
            fprintf(stderr, "error: --denoise: render settings %u (%s, min_samples %u) cannot take the adaptive path the statistics come from: %s\n", i,
                    naive ? "Naive renderer" : "Tiled renderer", rd.spp, why);
            return false;
        }
    }
    return true;
}

// ---- one [[render_settings]] entry: rendered, written and, with --denoise, filtered.  Every step returns success and has said on stderr what failed.

struct Pixels {   // what pt_output_film makes of a film
    std::vector<uint8_t> rgba;
    std::vector<float> linear;
    explicit Pixels(size_t np) : rgba(4 * np), linear(3 * np) {}
};

enum Mix { kMixResident, kMixResidentDenoised, kMixHost };   // where --light-gains mixes the group films: where the render, or the joint filter, left them, or from host arrays

struct Setting {
    const Run& r;
    const Options& o;
    pt_scene* const scene;
    const uint32_t index;
    pt_render_settings rs;
    pt_render_desc rd;
    pt_output_desc od;
    pt_guide_chain_desc cd;    // --guide-chain's descriptor, for every guide call of the setting
    pt_spectral_desc sd;       // the bins of --spectral-bins, --denoise-spectral-bins or --relamp-bins (only one of them is given)
    size_t np = 0;
    std::string base;          // <output-dir>/<filename>
    std::vector<float> film, spectral, group_films, group_bins;
    std::vector<uint32_t> counts;
    std::vector<double> stats;
    Pixels px{0};              // of the film, then of the denoised film: the spectral and Cryptomatte files written next carry its linear R, G, B

    Setting(const Run& run, uint32_t i) : r(run), o(run.o), scene(run.scene.get()), index(i) {}

    // The one render of the setting: picks the entry, prints the "rendering ..." line, calls it and names it when it fails.  A fixed count under --denoise goes
    // through the adaptive entries as --adaptive does (max_samples = min_samples, one round: pt_render's film bit for bit, and the statistics).
    bool render(pt_profile* prof, uint64_t* samples) {
        pt_config* config = r.config.get();
        // --adaptive: min_samples .. max_samples per pixel (pt_render_adaptive) where the setting gives a range and the renderer sums in phases of 10
        bool adaptive = o.adaptive >= 0.0f;
        pt_adaptive_desc ad = {0u, 0u, o.adaptive, 0.0f};
        if (adaptive) {
            uint32_t tw = 0, th = 0;
            if (pt_config_renderer(config, &tw, &th) == PT_RENDERER_NAIVE) {
                if (r.warnings) fprintf(stderr, "warning: --adaptive: render settings %u use the Naive renderer; rendering %u spp everywhere\n", index, rd.spp);
                adaptive = false;
            } else if (rs.max_samples < 0 || (uint32_t)rs.max_samples <= rd.spp) {
                if (r.warnings) fprintf(stderr, "warning: --adaptive: render settings %u have no max_samples > min_samples; rendering %u spp everywhere\n", index, rd.spp);
                adaptive = false;
            } else {
                const uint32_t lo = (rd.spp + 9u) / 10u * 10u, hi = ((uint32_t)rs.max_samples + 9u) / 10u * 10u;
                if ((lo != rd.spp || hi != (uint32_t)rs.max_samples) && r.warnings)
                    fprintf(stderr, "warning: --adaptive: samples %u..%d rounded up to %u..%u (multiples of 10)\n", rd.spp, rs.max_samples, lo, hi);
                rd.spp = lo; ad.max_samples = hi;
            }
        }
        const bool counted = adaptive || o.denoise;   // through the adaptive entries
        const pt_light_groups_desc* gd = &r.gd;
        const pt_path_passes_desc ppd = {{0u, 0u, 0u, 0u}};
        const uint32_t groups = o.path_passes ? (uint32_t)PT_PATH_PASSES : !o.path_exprs.empty() ? r.expr_program.outputs : (o.light_groups || o.denoise_groups) ? gd->group_count : 0u;
        film.resize(4 * np);
        counts.resize(counted ? np : 0);
        stats.resize(o.denoise ? 2 * np : 0);
        spectral.resize((size_t)(o.spectral_bins ? o.spectral_bins : o.denoise_bins) * np);
        group_films.resize((size_t)groups * 4 * np);
        group_bins.resize(o.relamp_groups ? (size_t)gd->group_count * o.relamp_bins * np : 0);
        float* const f = film.data();
        uint32_t* const n = counts.data();
        double* const st = stats.data();                             // (the spectral, group and pass entries always take the statistics)
        double* const st_plain = o.denoise ? stats.data() : nullptr;

        const char* entry = nullptr;
        std::function<pt_status()> call;
        std::string suffix;
        const auto pick = [&](const char* name, std::function<pt_status()> fn) { entry = name; call = std::move(fn); };
        if (counted) {
            if (o.denoise_bins && o.spectral_multi) pick("pt_render_adaptive_spectral_multi", [&] { return pt_render_adaptive_spectral_multi(scene, &rd, &ad, &sd, o.spectral_device_mask, f, n, st, spectral.data(), prof); });
            else if (o.denoise_bins) pick("pt_render_adaptive_spectral", [&] { return pt_render_adaptive_spectral(scene, &rd, &ad, &sd, f, n, st, spectral.data(), prof); });
            else if (o.denoise_groups && o.group_multi) pick("pt_render_adaptive_light_groups_multi", [&] { return pt_render_adaptive_light_groups_multi(scene, &rd, &ad, gd, o.group_device_mask, f, n, st, group_films.data(), prof); });
            else if (o.denoise_groups) pick("pt_render_adaptive_light_groups", [&] { return pt_render_adaptive_light_groups(scene, &rd, &ad, gd, f, n, st, group_films.data(), prof); });
            else if (o.denoise_passes) pick("pt_render_adaptive_path_passes", [&] { return pt_render_adaptive_path_passes(scene, &rd, &ad, &ppd, f, n, st, group_films.data(), prof); });
            else if (o.multi) pick("pt_render_adaptive_multi", [&] { return pt_render_adaptive_multi(scene, &rd, &ad, o.device_mask, f, n, st_plain, prof); });
            else pick("pt_render_adaptive", [&] { return pt_render_adaptive(scene, &rd, &ad, f, n, st_plain, prof); });
        } else if (o.spectral_bins) {
            if (o.spectral_multi) pick("pt_render_spectral_multi", [&] { return pt_render_spectral_multi(scene, &rd, &sd, o.spectral_device_mask, f, spectral.data(), prof); });
            else pick("pt_render_spectral", [&] { return pt_render_spectral(scene, &rd, &sd, f, spectral.data(), prof); });
        } else if (o.relamp_groups) {
            suffix = ", " + std::to_string(gd->group_count) + " light groups of " + std::to_string(o.relamp_bins) + " bins";
            pick("pt_render_light_groups_spectral", [&] { return pt_render_light_groups_spectral(scene, &rd, gd, &sd, f, nullptr, nullptr, group_bins.data(), prof); });
        } else if (o.path_passes) {
            suffix = ", " + std::to_string(PT_PATH_PASSES) + " path passes";
            pick("pt_render_path_passes", [&] { return pt_render_path_passes(scene, &rd, &ppd, f, group_films.data(), prof); });
        } else if (!o.path_exprs.empty()) {
            suffix = ", " + std::to_string(r.expr_program.outputs) + " path expressions";
            const uint8_t* ids = o.expr_groups ? r.instance_group.data() : nullptr;
            const uint32_t n_ids = o.expr_groups ? r.desc->instance_count : 0u;
            pick("pt_render_path_exprs", [this, ids, n_ids, f, prof] { return pt_render_path_exprs(scene, &rd, &r.expr_program, ids, n_ids, f, group_films.data(), prof); });
        } else if (o.light_groups) {
            suffix = ", " + std::to_string(gd->group_count) + " light groups";
            if (o.group_multi) pick("pt_render_light_groups_multi", [&] { return pt_render_light_groups_multi(scene, &rd, gd, o.group_device_mask, f, group_films.data(), prof); });
            else pick("pt_render_light_groups", [&] { return pt_render_light_groups(scene, &rd, gd, f, group_films.data(), prof); });
        } else if (o.multi) pick("pt_render_multi", [&] { return pt_render_multi(scene, &rd, o.device_mask, f, prof); });
        else pick("pt_render", [&] { return pt_render(scene, &rd, f, prof); });

        char spp[96] = " spp";
        if (adaptive) snprintf(spp, sizeof(spp), "..%u spp (adaptive, relative error %g)", ad.max_samples, (double)ad.rel_error);
        else if (counted) { ad.max_samples = rd.spp; ad.rel_error = 0.0f; }
        printf("rendering %ux%u, %u%s, max_bounces %u, light_samples %u%s\n", rd.width, rd.height, rd.spp, spp, rd.max_bounces, rd.light_samples, suffix.c_str());
        if (call() != PT_OK) return fail(entry);
        *samples = (uint64_t)rd.width * rd.height * rd.spp;
        if (adaptive) {
            uint32_t lo = 0xffffffffu, hi = 0;
            *samples = 0;
            for (uint32_t c : counts) { *samples += c; lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
            printf("adaptive: %.2f samples per pixel on average, min %u, max %u, %llu rounds\n", (double)*samples / (double)counts.size(), lo, hi,
                   (unsigned long long)prof->kernel_launches[5]);
        }
        return true;
    }

    // The one picture writer: a film through the setting's film output into `to`, then <stem>.exr, with `png` <stem>.png, and the "wrote ..." line with `note` in
    // parentheses.  `prefix` is the site's text in front of the engine's error; nullptr is the film itself, which names the stage that failed and, with
    // --write-film, also stores the film as <stem>.npy.
    bool write_picture(const float* xyzw, const std::string& stem, Pixels& to, bool png, const std::string& note, const char* prefix) {
        if (pt_output_film(&od, xyzw, to.rgba.data(), to.linear.data()) != PT_OK) return fail(prefix ? prefix : "pt_output_film");
        if (pt_write_exr((stem + ".exr").c_str(), rd.width, rd.height, to.linear.data(), od.colorspace) != PT_OK ||
            (png && pt_write_png((stem + ".png").c_str(), rd.width, rd.height, to.rgba.data(), od.colorspace) != PT_OK))
            return fail(prefix ? prefix : "failed to write files");   // the reference panics here (mod.rs:45-48)
        if (!prefix && o.write_film && !write_npy(stem + ".npy", xyzw, rd.height, rd.width)) { fprintf(stderr, "failed to write %s.npy\n", stem.c_str()); return false; }
        printf("wrote %s.exr", stem.c_str());
        if (png) printf(" and %s.png", stem.c_str());
        if (!note.empty()) printf(" (%s)", note.c_str());
        printf("\n");
        return true;
    }

    // --mattes: the ranked ids of this setting's frame (pt_render_mattes, beside the render: no other file changes) as a Cryptomatte file with the setting's linear
    // RGB — instances named instance<i>, materials by their names in the scene file's library
    bool write_mattes() {
        const pt_matte_desc md = {o.matte_samples ? o.matte_samples : (rs.min_samples < 65535u ? rs.min_samples : 65535u), o.matte_ranks,
                                  o.mattes == 2 ? (uint32_t)PT_MATTE_KEY_MATERIAL : (uint32_t)PT_MATTE_KEY_INSTANCE, {0u}};
        std::vector<uint32_t> m_keys(md.ranks * np), m_overflow(np), named;
        std::vector<float> m_coverage(md.ranks * np);
        if (pt_render_mattes(scene, &rd, &md, m_keys.data(), m_coverage.data(), m_overflow.data()) != PT_OK) return fail("pt_render_mattes");
        std::vector<std::string> names;
        for (uint32_t key : m_keys) {
            if (key == PT_MATTE_SKY || key == PT_MATTE_NONE) continue;
            bool seen = false;
            for (uint32_t k : named) seen = seen || k == key;
            if (seen) continue;
            const char* material = o.mattes == 2 ? pt_scene_file_material_name(r.scene_file.get(), key) : nullptr;
            named.push_back(key);
            names.push_back(o.mattes == 1 ? "instance" + std::to_string(key) : material ? std::string(material) : "key" + std::to_string(key));
        }
        std::vector<const char*> name_ptrs;
        for (const std::string& s : names) name_ptrs.push_back(s.c_str());
        uint64_t dropped = 0;
        for (uint32_t c : m_overflow) dropped += c;
        const std::string crypto = base + "_crypto.exr";
        if (pt_write_exr_cryptomatte(crypto.c_str(), rd.width, rd.height, md.ranks, m_keys.data(), m_coverage.data(), o.mattes == 2 ? "CryptoMaterial" : "CryptoObject",
                                     (uint32_t)named.size(), named.data(), name_ptrs.data(), px.linear.data(), od.colorspace) != PT_OK)
            return fail(("failed to write " + crypto).c_str());
        printf("wrote %s (%u ranks of %u samples, %zu names, %llu samples beyond the ranks)\n", crypto.c_str(), md.ranks, md.samples, names.size(), (unsigned long long)dropped);
        return true;
    }

    // --light-groups, --denoise-light-groups: every group's film, and with --light-gains their mix, through this setting's film output (buffers of their own).
    // `stem`: base, or base + "_denoised" for the films of the joint filter.
    bool write_groups(const std::string& stem, const std::vector<float>& films, Mix mix) {
        const uint32_t groups = r.gd.group_count;
        Pixels own(np);
        for (uint32_t g = 0; g < groups; ++g)
            if (!write_picture(films.data() + 4 * np * g, stem + "_light" + std::to_string(g), own, false, "", r.group_flag)) return false;
        if (!o.has_light_gains) return true;
        std::vector<float> matrices, relit(4 * np);
        for (float gain : o.light_gains) for (int k = 0; k < 9; ++k) matrices.push_back(k % 4 == 0 ? gain : 0.0f);
        const pt_status st = mix == kMixHost              ? pt_light_groups_mix(rd.width, rd.height, groups, films.data(), matrices.data(), relit.data())
                             : mix == kMixResidentDenoised ? pt_light_groups_mix_resident_denoised(scene, matrices.data(), relit.data())
                                                           : pt_light_groups_mix_resident(scene, matrices.data(), relit.data());
        if (st != PT_OK) return fail(r.group_flag);
        return write_picture(relit.data(), stem + "_relit", own, true, "relit from " + std::to_string(groups) + " light groups", r.group_flag);
    }

    // --path-passes: every class's film through this setting's film output (buffers of their own).  `stem`: base, or base + "_denoised"
    bool write_passes(const std::string& stem, const std::vector<float>& films) {
        Pixels own(np);
        for (int c = 0; c < PT_PATH_PASSES; ++c)
            if (!write_picture(films.data() + 4 * np * c, stem + "_pass_" + kPathPassNames[c], own, false, "", "--path-passes")) return false;
        return true;
    }

    // --path-exprs: every expression's film through this setting's film output (buffers of their own)
    bool write_exprs(const std::vector<float>& films) {
        Pixels own(np);
        for (size_t e = 0; e < o.path_exprs.size(); ++e)
            if (!write_picture(films.data() + 4 * np * e, base + "_expr_" + o.path_exprs[e].first, own, false, "", "--path-exprs")) return false;
        return true;
    }

    // --relamp-groups: every group's bins in the units of the EXR payload, and the re-lamped picture — the colour-matching development of the group bins by the
    // re-lamp matrix, where the render left them on the device — through this setting's film output (buffers of its own)
    bool write_relamped() {
        const uint32_t groups = r.gd.group_count;
        const size_t plane = (size_t)o.relamp_bins * np;
        std::vector<float> centres(o.relamp_bins), scaled(plane), matrix((size_t)3 * groups * o.relamp_bins), planes(3 * np);
        if (pt_spectral_bin_centres(&rd, &sd, centres.data()) != PT_OK) return fail("--relamp-groups");
        for (uint32_t g = 0; g < groups; ++g) {
            const std::string name = base + "_light" + std::to_string(g) + "_spectral";
            for (size_t k = 0; k < plane; ++k) scaled[k] = group_bins[plane * g + k] * od.factor;
            if (pt_write_exr_spectral((name + ".exr").c_str(), rd.width, rd.height, o.relamp_bins, centres.data(), scaled.data(), nullptr, od.colorspace) != PT_OK) return fail("--relamp-groups");
            printf("wrote %s.exr (%u bins)\n", name.c_str(), o.relamp_bins);
        }
        const int32_t cie[3] = {PT_RESPONSE_CIE_X, PT_RESPONSE_CIE_Y, PT_RESPONSE_CIE_Z};
        const Curves& c = r.relamp_curves;
        if (pt_light_groups_relamp_matrix(&rd, &sd, c.curves.data(), (uint32_t)c.curves.size(), c.data.data(), (uint32_t)c.data.size(), 3, cie, PT_SPECTRAL_NO_FILTER,
                                          o.develop_subsamples, groups, r.relamp_old.data(), r.relamp_new.data(), o.has_relamp_gains ? o.relamp_gains.data() : nullptr,
                                          matrix.data()) != PT_OK ||
            pt_light_groups_relamp_resident(scene, 3, matrix.data(), planes.data()) != PT_OK)
            return fail("--relamp-groups");
        Pixels own(np);
        return write_picture(pack_planes(planes, np).data(), base + "_relamped", own, true,
                             "re-lamped from " + std::to_string(groups) + " light groups of " + std::to_string(o.relamp_bins) + " bins", "--relamp-groups");
    }

    // <name>.exr: the bins in the units of the EXR payload — the same factor, applied here in place, one multiply per value — beside the R, G, B of the picture
    // written last into `px`
    bool write_spectral(const std::string& name, std::vector<float>& scaled) {
        std::vector<float> centres(sd.bins);
        for (float& v : scaled) v *= od.factor;
        if (pt_spectral_bin_centres(&rd, &sd, centres.data()) != PT_OK ||
            pt_write_exr_spectral((name + ".exr").c_str(), rd.width, rd.height, sd.bins, centres.data(), scaled.data(), px.linear.data(), od.colorspace) != PT_OK)
            return fail(o.spectral_bins ? "--spectral-bins" : "--denoise-spectral-bins");
        printf("wrote %s.exr (%u bins)\n", name.c_str(), sd.bins);
        return true;
    }

    // --develop: three planes from the bins — the scene's resident ones (bins == nullptr; `denoised`: the resident denoised ones) or a host array as rendered or
    // filtered, before the factor —, packed as an XYZW film with W = 0, through this setting's film output (buffers of its own: `px` still serves the spectral files)
    bool develop(const std::string& name, const float* bins, bool denoised) {
        const Curves& c = r.develop_curves;
        std::vector<float> matrix((size_t)3 * sd.bins), planes(3 * np);
        pt_status st = pt_spectral_response_matrix(&rd, &sd, c.curves.data(), (uint32_t)c.curves.size(), c.data.data(), (uint32_t)c.data.size(), 3, r.develop_responses,
                                                   r.develop_filter, o.develop_subsamples, matrix.data());
        if (st == PT_OK) st = bins       ? pt_spectral_project(rd.width, rd.height, sd.bins, 3, matrix.data(), bins, planes.data())
                              : denoised ? pt_spectral_project_resident_denoised(scene, 3, matrix.data(), planes.data())
                                         : pt_spectral_project_resident(scene, 3, matrix.data(), planes.data());
        if (st != PT_OK) return fail("--develop");
        Pixels own(np);
        return write_picture(pack_planes(planes, np).data(), name, own, true, "developed from " + std::to_string(sd.bins) + " bins", "--develop");
    }

    // The guides over host arrays: `albedo` with --demodulate-albedo, `bin_albedo` too with --demodulate-bins (else nullptr).
    pt_status host_guides(float* guides, float* albedo, float* bin_albedo) {
        return bin_albedo ? pt_render_guides_bin_albedo(scene, &rd, o.guide_samples, o.chain ? &cd : nullptr, o.denoise_bins, guides, albedo, bin_albedo)
               : o.chain  ? pt_render_guides_chain(scene, &rd, o.guide_samples, &cd, guides, albedo)
               : albedo   ? pt_render_guides_albedo(scene, &rd, o.guide_samples, guides, albedo)
                          : pt_render_guides(scene, &rd, o.guide_samples, guides);
    }

    // The guides beside what the render left on the device.
    pt_status resident_guides() {
        const uint32_t parts = o.demodulate_bins ? (PT_RESIDENT_ALBEDO | PT_RESIDENT_BIN_ALBEDO) : o.demodulate ? PT_RESIDENT_ALBEDO : 0u;
        return pt_resident_guides(scene, &rd, o.guide_samples, o.chain ? &cd : nullptr, parts);
    }

    pt_denoise_desc host_denoise_desc(uint64_t mask) const {   // the default filter on the first device of the mask: where a node render's gather left the film
        pt_denoise_desc dd;
        memset(&dd, 0, sizeof(dd));
        dd.width = rd.width; dd.height = rd.height; dd.device = first_device(mask);
        return dd;
    }

    // --denoise: four routes to `clean` — host arrays of a node group render; the resident group or pass films; the resident or assembled film and bins; host
    // arrays — with their own guide and filter calls, then <base>_denoised.* from it and what the route's flags add.
    bool denoise() {
        if (o.assemble) {
            // the node render left its pieces on the devices: one film on the scene's device from them, unless the mask came down to that device alone and
            // the render left the film resident itself
            struct pt_resident_info now;
            pt_status ast = pt_resident_info(scene, &now);
            if (ast == PT_OK && !(now.parts & PT_RESIDENT_FILM)) ast = pt_resident_assemble(scene, 0u);
            if (ast != PT_OK) return fail("--denoise-assemble");
        }
        // (a node group render without --denoise-assemble left no film one device can filter, unless the mask came down to the scene's device alone)
        bool groups_on_host = false;
        if (o.denoise_groups && o.group_multi && !o.assemble) {
            struct pt_resident_info now;
            if (pt_resident_info(scene, &now) != PT_OK) return fail("--light-group-devices");
            groups_on_host = !(now.parts & PT_RESIDENT_FILM);
        }
        const std::string dbase = base + "_denoised";
        const auto write_clean = [&](const std::vector<float>& clean) { return write_picture(clean.data(), dbase, px, true, "", nullptr); };
        std::vector<float> clean(4 * np);
        pt_resident_denoise_desc rdd;
        memset(&rdd, 0, sizeof(rdd));
        if (groups_on_host) {
            // guides and the joint filter over host arrays, on the first device of the mask: the files of the resident route, byte for byte
            std::vector<float> guides(4 * np), albedo(o.demodulate ? 4 * np : 0), clean_groups(4 * np * r.gd.group_count);
            float* const alb = o.demodulate ? albedo.data() : nullptr;
            const pt_denoise_desc dd = host_denoise_desc(o.group_device_mask);
            pt_status st = host_guides(guides.data(), alb, nullptr);
            if (st == PT_OK) st = pt_denoise_light_groups(&dd, r.gd.group_count, film.data(), counts.data(), stats.data(), guides.data(), alb, group_films.data(), clean.data(),
                                                          nullptr, clean_groups.data());
            if (st != PT_OK) return fail("--denoise-light-groups");
            return write_clean(clean) && write_groups(dbase, clean_groups, kMixHost);
        }
        if (o.denoise_groups || o.denoise_passes) {
            // the render left the film, its statistics and the group films on the device, paired: the guides stay there too, and the joint filter runs on all of
            // it (with or without --denoise-resident: this is the only route, and its files are those of either)
            // (--denoise-path-passes: the pass films are the resident group films of this route)
            std::vector<float> clean_groups(4 * np * (o.denoise_passes ? (uint32_t)PT_PATH_PASSES : r.gd.group_count));
            pt_status st = resident_guides();
            if (st == PT_OK) st = pt_denoise_light_groups_resident(scene, &rdd, clean.data(), nullptr, clean_groups.data());
            if (st != PT_OK) return fail(o.denoise_passes ? "--denoise-path-passes" : "--denoise-light-groups");
            return write_clean(clean) && (o.denoise_passes ? write_passes(dbase, clean_groups) : write_groups(dbase, clean_groups, kMixResidentDenoised));
        }
        std::vector<float> clean_spectral(spectral.size());
        const bool on_device = o.resident || o.assemble;
        if (on_device) {
            // the render left film, counts, statistics and bins on the device: the guides stay there too, and the filter runs on all of it
            pt_status st = resident_guides();
            if (st == PT_OK) st = pt_denoise_resident(scene, &rdd, clean.data(), nullptr, o.denoise_bins ? clean_spectral.data() : nullptr);
            if (st != PT_OK) return fail(o.assemble ? "--denoise-assemble" : "--denoise-resident");
        } else {
            const bool with_albedo = o.demodulate || o.demodulate_bins;
            std::vector<float> guides(4 * np), albedo(with_albedo ? 4 * np : 0), bin_albedo(o.demodulate_bins ? spectral.size() : 0);
            float* const alb = with_albedo ? albedo.data() : nullptr;
            const pt_denoise_desc dd = host_denoise_desc(o.multi ? o.device_mask : o.spectral_multi ? o.spectral_device_mask : 0);
            pt_status st = host_guides(guides.data(), alb, o.demodulate_bins ? bin_albedo.data() : nullptr);
            if (st == PT_OK)
                st = o.demodulate_bins ? pt_denoise_spectral_albedo(&dd, o.denoise_bins, film.data(), counts.data(), stats.data(), guides.data(), alb, spectral.data(),
                                                                    bin_albedo.data(), clean.data(), clean_spectral.data(), nullptr)
                     : o.denoise_bins  ? pt_denoise_spectral(&dd, o.denoise_bins, film.data(), counts.data(), stats.data(), guides.data(), spectral.data(), clean.data(),
                                                             clean_spectral.data(), nullptr)
                                       : pt_denoise_film_albedo(&dd, film.data(), counts.data(), stats.data(), guides.data(), alb, clean.data(), nullptr);
            if (st != PT_OK) return fail("--denoise");
        }
        if (!write_clean(clean)) return false;
        // the denoised bins are developed before the factor goes into them, and their file carries the denoised film's R, G, B, which `px` now holds
        if (o.develop && o.denoise_bins && !develop(dbase + "_developed", on_device ? nullptr : clean_spectral.data(), true)) return false;
        return !o.denoise_bins || write_spectral(dbase + "_spectral", clean_spectral);
    }

    bool run() {
        if (o.hero) rd.hero_wavelengths = o.hero;   // engine extension (not in the reference's files): 4 wavelengths per path
        np = (size_t)rd.width * rd.height;
        memset(&cd, 0, sizeof(cd));
        cd.max_chain = o.max_chain; cd.alpha_max = o.alpha_max;
        sd = {o.spectral_bins ? o.spectral_bins : o.denoise_bins ? o.denoise_bins : o.relamp_bins, {0u, 0u, 0u}};
        pt_profile prof;
        uint64_t samples = 0;
        if (!render(&prof, &samples)) return false;
        // Profile::pretty_print (src/profile.rs:20-34)
        const double total = (double)(prof.camera_rays + prof.bounce_rays + prof.shadow_rays + prof.light_rays);
        printf("took %.3fs\n", prof.seconds);
        printf("%llu camera rays, %llu bounce rays, %llu shadow rays, %llu light rays, %llu environment hits\n", (unsigned long long)prof.camera_rays,
               (unsigned long long)prof.bounce_rays, (unsigned long long)prof.shadow_rays, (unsigned long long)prof.light_rays, (unsigned long long)prof.env_hits);
        printf("%.1f rays per second, %.3f Msamples/s\n", total / prof.seconds, (double)samples / prof.seconds * 1e-6);
        pt_config_output_desc(r.config.get(), index, 1.0f, &od);
        px = Pixels(np);
        base = o.output_dir + "/" + (rs.filename ? rs.filename : "beauty");  // src/renderer/mod.rs:27-31
        if (!write_picture(film.data(), base, px, true, "", nullptr)) return false;
        if (o.mattes && !write_mattes()) return false;
        if (r.group_mode && !o.relamp_groups && o.path_exprs.empty() && !write_groups(base, group_films, kMixResident)) return false;
        if (o.path_passes && !write_passes(base, group_films)) return false;
        if (!o.path_exprs.empty() && !write_exprs(group_films)) return false;
        if (o.relamp_groups && !write_relamped()) return false;
        if (o.denoise_bins) {   // (a copy: the filter takes the bins as rendered)
            std::vector<float> noisy(spectral);
            if (!write_spectral(base + "_spectral", noisy)) return false;
        } else if (!spectral.empty() && !write_spectral(base + "_spectral", spectral)) return false;
        // (a node render leaves its bins resident too, with either flag: they are developed on the devices)
        if (o.develop && !develop(base + "_developed", o.denoise_bins && !o.spectral_multi && !o.resident ? spectral.data() : nullptr, false)) return false;
        return !o.denoise || denoise();
    }
};

// Every [[render_settings]] entry in turn; the first that fails ends the run.
bool render_settings(Run& r) {
    pt_scene* scene = nullptr;
    if (pt_scene_create(r.desc, &scene) != PT_OK) return fail("pt_scene_create");
    r.scene.reset(scene);
    const uint32_t n = pt_config_render_settings_count(r.config.get());
    for (uint32_t i = 0; i < n; ++i) {
        Setting s(r, i);
        pt_config_render_settings(r.config.get(), i, &s.rs);
        if (pt_config_render_desc(r.config.get(), i, r.o.seed, &s.rd) != PT_OK) {
            // the reference skips render settings whose integrator it cannot construct (src/renderer/tiled.rs:560-566)
            fprintf(stderr, "skipping render settings %u: %s\n", i, pt_scene_file_last_error());
            continue;
        }
        if (!s.run()) return false;
    }
    printf("render done\n");
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    Run r;
    Options& o = r.o;
    bool help = false;
    std::string mistake = parse_options(argc, argv, o, &help);
    if (help) { usage(""); return 0; }
    if (mistake.empty()) mistake = check_options(o);
    if (!mistake.empty()) return usage(mistake);
    const bool verbose = o.stdout_log_level == "info" || o.stdout_log_level == "debug" || o.stdout_log_level == "trace";
    r.warnings = verbose || o.stdout_log_level == "warn";
    if (!o.root.empty()) pt_scene_file_set_root(o.root.c_str());

    pt_config* config = nullptr;
    if (pt_config_load(o.config.c_str(), &config) != PT_OK) {
        fprintf(stderr, "couldn't read config.toml, %s\n", pt_scene_file_last_error());   // main.rs:115-121
        return 1;
    }
    r.config.reset(config);
    std::string scene_path = o.has_scene ? o.scene : pt_config_scene_file(config);        // main.rs:133
    pt_scene_file* scene_file = nullptr;
    if (pt_scene_file_load(scene_path.c_str(), config, &scene_file) != PT_OK) {
        fprintf(stderr, "failed to construct the scene: %s\n", pt_scene_file_last_error());  // main.rs:139-149
        return 1;
    }
    r.scene_file.reset(scene_file);
    if (r.warnings) for (uint32_t k = 0; k < pt_scene_file_warning_count(scene_file); ++k) fprintf(stderr, "warning: %s\n", pt_scene_file_warning(scene_file, k));
    const pt_scene_desc* desc = r.desc = pt_scene_file_desc(scene_file);
    if (verbose) printf("scene %s: %u instances, %u meshes, %zu triangles, %u materials, %u curves\n", scene_path.c_str(), desc->instance_count, desc->mesh_count,
                        desc->index_count / 3, desc->material_count, desc->curve_count);

    if (o.develop && !load_develop_curves(r)) return 1;
    r.instance_group.assign(desc->instance_count, 0);
    memset(&r.gd, 0, sizeof(r.gd));
    r.group_mode = o.light_groups ? o.light_groups : o.denoise_groups ? o.denoise_groups : o.relamp_groups ? o.relamp_groups : o.expr_groups;
    r.group_flag = o.light_groups ? "--light-groups" : o.denoise_groups ? "--denoise-light-groups" : o.relamp_groups ? "--relamp-groups" : "--path-expr-groups";
    if (r.group_mode && !form_light_groups(r)) return 1;
    if (o.path_passes) {
        printf("path passes: %d (", PT_PATH_PASSES);
        for (int c = 0; c < PT_PATH_PASSES; ++c) printf("%s%s", c ? ", " : "", kPathPassNames[c]);
        printf(")\n");
    }
    if (!o.path_exprs.empty()) {
        const std::string mistake = compile_path_exprs(o.path_exprs, r.gd.environment_group, &r.expr_program);
        if (!mistake.empty()) { fprintf(stderr, "error: --path-exprs: %s\n", mistake.c_str()); return 1; }
        printf("path expressions: %u (", r.expr_program.outputs);
        for (size_t e = 0; e < o.path_exprs.size(); ++e) printf("%s%s", e ? ", " : "", o.path_exprs[e].first.c_str());
        printf("), %u states\n", r.expr_program.states);
    }
    if (o.relamp_groups && !load_relamp_curves(r)) return 1;
    if (o.denoise && !o.dry_run && !adaptive_path_takes_every_setting(r)) return 1;

    printf("constructing renderer\n");
    mkdir(o.output_dir.c_str(), 0777);                                                     // main.rs:155-158
    return o.dry_run || render_settings(r) ? 0 : 1;
}
