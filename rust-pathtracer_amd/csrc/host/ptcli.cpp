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
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
};

const char* const kPathPassNames[PT_PATH_PASSES] = {"emission", "background", "diffuse_direct", "diffuse_indirect", "reflection_direct", "reflection_indirect",
                                                    "transmission_direct", "transmission_indirect"};

int usage(const char* msg) {
    if (msg) fprintf(stderr, "error: %s\n", msg);
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
                    "             [--path-passes] [--denoise-path-passes]\n");
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

}  // namespace

int main(int argc, char** argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto value = [&](std::string* dst) { if (i + 1 >= argc) return false; *dst = argv[++i]; return true; };
        std::string v;
        if (a == "--config") { if (!value(&o.config)) return usage("--config needs a value"); }
        else if (a == "--scene") { if (!value(&o.scene)) return usage("--scene needs a value"); o.has_scene = true; }
        else if (a == "-n" || a == "--dry-run") o.dry_run = true;
        else if (a == "--stdout-log-level") { if (!value(&o.stdout_log_level)) return usage("--stdout-log-level needs a value"); }
        else if (a == "--write-log-level") { if (!value(&v)) return usage("--write-log-level needs a value"); }
        else if (a == "--root") { if (!value(&o.root)) return usage("--root needs a value"); }
        else if (a == "--output-dir") { if (!value(&o.output_dir)) return usage("--output-dir needs a value"); }
        else if (a == "--seed") { if (!value(&v)) return usage("--seed needs a value"); o.seed = strtoull(v.c_str(), nullptr, 10); }
        else if (a == "--write-film") o.write_film = true;
        else if (a == "--hero-wavelengths") { if (!value(&v)) return usage("--hero-wavelengths needs a value"); o.hero = (uint32_t)strtoul(v.c_str(), nullptr, 10); }
        else if (a == "--adaptive") {
            if (!value(&v)) return usage("--adaptive needs a value");
            char* end = nullptr;
            o.adaptive = strtof(v.c_str(), &end);
            if (end == v.c_str() || *end || !(o.adaptive >= 0.0f)) return usage("--adaptive needs a relative error >= 0");
        }
        else if (a == "--devices") {
            if (!value(&v)) return usage("--devices needs a value");
            char* end = nullptr;
            o.device_mask = strtoull(v.c_str(), &end, 0);
            if (end == v.c_str() || *end) return usage("--devices needs a device mask (bit d = HIP device d, 0 = all)");
            o.multi = true;
        }
        else if (a == "--denoise") o.denoise = true;
        else if (a == "--demodulate-albedo") o.demodulate = true;
        else if (a == "--demodulate-bins") o.demodulate_bins = true;
        else if (a == "--denoise-resident") o.resident = true;
        else if (a == "--denoise-assemble") o.assemble = true;
        else if (a == "--guide-samples") {
            if (!value(&v)) return usage("--guide-samples needs a value");
            char* end = nullptr;
            o.guide_samples = (uint32_t)strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || o.guide_samples == 0) return usage("--guide-samples needs a positive count");
        }
        else if (a == "--guide-chain") {
            if (!value(&v)) return usage("--guide-chain needs a value");
            char* end = nullptr;
            o.max_chain = (uint32_t)strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || o.max_chain > PT_GUIDE_CHAIN_MAX) return usage("--guide-chain needs a count of at most 16");
            o.chain = true;
        }
        else if (a == "--guide-alpha-max") {
            if (!value(&v)) return usage("--guide-alpha-max needs a value");
            char* end = nullptr;
            o.alpha_max = strtof(v.c_str(), &end);
            if (end == v.c_str() || *end || !(o.alpha_max >= 0.0f) || !(o.alpha_max < 1e30f)) return usage("--guide-alpha-max needs a finite alpha >= 0");
            o.has_alpha_max = true;
        }
        else if (a == "--spectral-bins") {
            if (!value(&v)) return usage("--spectral-bins needs a value");
            char* end = nullptr;
            const unsigned long b = strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || b == 0 || b > PT_SPECTRAL_MAX_BINS) return usage("--spectral-bins needs a count in 1..64");
            o.spectral_bins = (uint32_t)b;
        }
        else if (a == "--denoise-spectral-bins") {
            if (!value(&v)) return usage("--denoise-spectral-bins needs a value");
            char* end = nullptr;
            const unsigned long b = strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || b == 0 || b > PT_SPECTRAL_MAX_BINS) return usage("--denoise-spectral-bins needs a count in 1..64");
            o.denoise_bins = (uint32_t)b;
        }
        else if (a == "--develop") {
            if (!value(&v)) return usage("--develop needs a value");
            o.develop_curves.clear();
            if (v != "cie") {
                size_t p = 0;
                while (true) {
                    const size_t c = v.find(',', p);
                    o.develop_curves.push_back(v.substr(p, c == std::string::npos ? std::string::npos : c - p));
                    if (c == std::string::npos) break;
                    p = c + 1;
                }
                bool ok = o.develop_curves.size() == 3;
                for (const std::string& n : o.develop_curves) ok = ok && !n.empty();
                if (!ok) return usage("--develop needs `cie` or three curve names CX,CY,CZ");
            }
            o.develop = true;
        }
        else if (a == "--develop-filter") {
            if (!value(&o.develop_filter) || o.develop_filter.empty()) return usage("--develop-filter needs a curve name");
            o.has_develop_filter = true;
        }
        else if (a == "--develop-subsamples") {
            if (!value(&v)) return usage("--develop-subsamples needs a value");
            char* end = nullptr;
            const unsigned long n = strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || n == 0 || n > PT_SPECTRAL_MAX_SUBSAMPLES) return usage("--develop-subsamples needs a count in 1..16");
            o.develop_subsamples = (uint32_t)n; o.has_develop_subsamples = true;
        }
        else if (a == "--spectral-devices") {
            if (!value(&v)) return usage("--spectral-devices needs a value");
            char* end = nullptr;
            o.spectral_device_mask = strtoull(v.c_str(), &end, 0);
            if (end == v.c_str() || *end) return usage("--spectral-devices needs a device mask (bit d = HIP device d, 0 = all)");
            o.spectral_multi = true;
        }
        else if (a == "--light-group-devices") {
            if (!value(&v)) return usage("--light-group-devices needs a value");
            char* end = nullptr;
            o.group_device_mask = strtoull(v.c_str(), &end, 0);
            if (end == v.c_str() || *end) return usage("--light-group-devices needs a device mask (bit d = HIP device d, 0 = all)");
            o.group_multi = true;
        }
        else if (a == "--light-groups") {
            if (!value(&v)) return usage("--light-groups needs a value");
            o.light_groups = v == "instance" ? 1 : v == "material" ? 2 : 0;
            if (!o.light_groups) return usage("--light-groups needs `instance` or `material`");
        }
        else if (a == "--relamp-groups") {
            if (!value(&v)) return usage("--relamp-groups needs a value");
            o.relamp_groups = v == "instance" ? 1 : v == "material" ? 2 : 0;
            if (!o.relamp_groups) return usage("--relamp-groups needs `instance` or `material`");
        }
        else if (a == "--relamp-bins") {
            if (!value(&v)) return usage("--relamp-bins needs a value");
            char* end = nullptr;
            const unsigned long b = strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || b == 0 || b > PT_SPECTRAL_MAX_BINS) return usage("--relamp-bins needs a count in 1..64");
            o.relamp_bins = (uint32_t)b;
        }
        else if (a == "--relamp") {
            if (!value(&v)) return usage("--relamp needs a value");
            o.has_relamp = true;
            o.relamp.clear();
            size_t p = 0;
            while (true) {
                const size_t c = v.find(',', p);
                const std::string item = v.substr(p, c == std::string::npos ? std::string::npos : c - p);
                const size_t colon = item.find(':');
                char* end = nullptr;
                const unsigned long g = strtoul(item.c_str(), &end, 10);
                if (colon == std::string::npos || colon == 0 || end != item.c_str() + colon || colon + 1 >= item.size() || g >= PT_LIGHT_GROUPS_MAX)
                    return usage("--relamp needs G:CURVE[,G:CURVE...] with G a group in 0..7");
                for (const auto& have : o.relamp) if (have.first == (uint32_t)g) return usage("--relamp names a group twice");
                o.relamp.push_back({(uint32_t)g, item.substr(colon + 1)});
                if (c == std::string::npos) break;
                p = c + 1;
            }
        }
        else if (a == "--relamp-gains") {
            if (!value(&v)) return usage("--relamp-gains needs a value");
            o.has_relamp_gains = true;
            o.relamp_gains.clear();
            size_t p = 0;
            while (true) {
                const size_t c = v.find(',', p);
                const std::string item = v.substr(p, c == std::string::npos ? std::string::npos : c - p);
                char* end = nullptr;
                const float g = strtof(item.c_str(), &end);
                if (item.empty() || end == item.c_str() || *end || !(g > -1e30f && g < 1e30f)) return usage("--relamp-gains needs finite gains g0,g1,...");
                o.relamp_gains.push_back(g);
                if (c == std::string::npos) break;
                p = c + 1;
            }
            if (o.relamp_gains.size() > PT_LIGHT_GROUPS_MAX) return usage("--relamp-gains takes at most 8 gains");
        }
        else if (a == "--denoise-light-groups") {
            if (!value(&v)) return usage("--denoise-light-groups needs a value");
            o.denoise_groups = v == "instance" ? 1 : v == "material" ? 2 : 0;
            if (!o.denoise_groups) return usage("--denoise-light-groups needs `instance` or `material`");
        }
        else if (a == "--light-gains") {
            if (!value(&v)) return usage("--light-gains needs a value");
            o.has_light_gains = true;
            o.light_gains.clear();
            for (size_t at = 0; at <= v.size();) {
                const size_t comma = v.find(',', at);
                const std::string item = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
                char* end = nullptr;
                const float g = strtof(item.c_str(), &end);
                if (item.empty() || end == item.c_str() || *end || !(g > -1e30f && g < 1e30f)) return usage("--light-gains needs finite gains G0,G1,...");
                o.light_gains.push_back(g);
                if (comma == std::string::npos) break;
                at = comma + 1;
            }
            if (o.light_gains.size() > PT_LIGHT_GROUPS_MAX) return usage("--light-gains takes at most 8 gains");
        }
        else if (a == "--mattes") {
            if (!value(&v)) return usage("--mattes needs a value");
            o.mattes = v == "instance" ? 1 : v == "material" ? 2 : 0;
            if (!o.mattes) return usage("--mattes needs `instance` or `material`");
        }
        else if (a == "--matte-ranks" || a == "--matte-samples") {
            if (!value(&v)) return usage((a + " needs a value").c_str());
            char* end = nullptr;
            const unsigned long x = strtoul(v.c_str(), &end, 10);
            const bool ranks = a == "--matte-ranks";
            if (end == v.c_str() || *end || x == 0 || x > (ranks ? (unsigned long)PT_MATTE_RANKS_MAX : 65535ul))
                return usage(ranks ? "--matte-ranks needs a number of ranks in 1..8" : "--matte-samples needs a number of samples in 1..65535");
            (ranks ? o.matte_ranks : o.matte_samples) = (uint32_t)x;
            (ranks ? o.has_matte_ranks : o.has_matte_samples) = true;
        }
        else if (a == "--path-passes") o.path_passes = true;
        else if (a == "--denoise-path-passes") o.denoise_passes = true;
        else if (a == "-h" || a == "--help") { usage(nullptr); return 0; }
        else return usage(("unknown option " + a).c_str());
    }
    if (o.denoise_passes && !(o.path_passes && o.denoise)) return usage("--denoise-path-passes needs --path-passes and --denoise");
    if (o.path_passes) {
        const char* with = (o.adaptive >= 0.0f && !o.denoise_passes) ? "--adaptive" : o.spectral_bins ? "--spectral-bins" : o.denoise_bins ? "--denoise-spectral-bins"
                         : o.multi ? "--devices" : o.spectral_multi ? "--spectral-devices" : o.hero ? "--hero-wavelengths" : o.light_groups ? "--light-groups"
                         : o.denoise_groups ? "--denoise-light-groups" : o.relamp_groups ? "--relamp-groups" : o.group_multi ? "--light-group-devices"
                         : o.assemble ? "--denoise-assemble" : nullptr;
        static std::string refusal;
        if (with) { refusal = std::string("--path-passes cannot be combined with ") + with + ": a pass render is one render of one wavelength per path on one device, and its films are the scene's resident group films"; return usage(refusal.c_str()); }
        if (o.denoise && !o.denoise_passes) return usage("--path-passes cannot be combined with --denoise without --denoise-path-passes: the filter of the pass films takes the adaptive pass render");
    }
    if (o.group_multi && !o.light_groups && !o.denoise_groups) return usage("--light-group-devices needs --light-groups or --denoise-light-groups: it names the devices their group render runs on");
    if (o.group_multi && o.multi) return usage("--light-group-devices cannot be combined with --devices: a group render takes its devices from --light-group-devices alone");
    if (o.relamp_groups) {
        const char* with = o.adaptive >= 0.0f ? "--adaptive" : o.denoise ? "--denoise" : o.light_groups ? "--light-groups" : o.spectral_bins ? "--spectral-bins"
                         : o.denoise_bins ? "--denoise-spectral-bins" : o.multi ? "--devices" : o.spectral_multi ? "--spectral-devices" : o.hero ? "--hero-wavelengths" : nullptr;
        static std::string refusal;
        if (with) { refusal = std::string("--relamp-groups cannot be combined with ") + with + ": a spectral group render is one plain render of one wavelength per path on one device"; return usage(refusal.c_str()); }
        if (!o.relamp_bins) return usage("--relamp-groups needs --relamp-bins");
    } else {
        if (o.relamp_bins) return usage("--relamp-bins needs --relamp-groups");
        if (o.has_relamp) return usage("--relamp needs --relamp-groups");
        if (o.has_relamp_gains) return usage("--relamp-gains needs --relamp-groups");
    }
    if (o.denoise_groups) {
        const char* with = o.light_groups ? "--light-groups" : o.spectral_bins ? "--spectral-bins" : o.denoise_bins ? "--denoise-spectral-bins" : o.multi ? "--devices"
                         : o.spectral_multi ? "--spectral-devices" : (o.assemble && !o.group_multi) ? "--denoise-assemble" : o.hero ? "--hero-wavelengths" : nullptr;
        static std::string refusal;
        if (with) { refusal = std::string("--denoise-light-groups cannot be combined with ") + with + ": it is one adaptive group render of one wavelength per path on one device, and its filter"; return usage(refusal.c_str()); }
        if (!o.denoise) return usage("--denoise-light-groups needs --denoise");
    }
    if (o.has_light_gains && !o.light_groups && !o.denoise_groups) return usage("--light-gains needs --light-groups");
    if (o.light_groups) {
        const char* with = o.adaptive >= 0.0f ? "--adaptive" : o.denoise ? "--denoise" : o.spectral_bins ? "--spectral-bins" : o.denoise_bins ? "--denoise-spectral-bins"
                         : o.multi ? "--devices" : o.spectral_multi ? "--spectral-devices" : o.hero ? "--hero-wavelengths" : nullptr;
        static std::string refusal;
        if (with) { refusal = std::string("--light-groups cannot be combined with ") + with + ": a group render is one plain render of one wavelength per path on one device"; return usage(refusal.c_str()); }
    }
    if (o.mattes) {
        const char* with = o.multi ? "--devices" : o.spectral_multi ? "--spectral-devices" : o.group_multi ? "--light-group-devices" : nullptr;
        static std::string refusal;
        if (with) { refusal = std::string("--mattes cannot be combined with ") + with + ": a matte render runs on the scene's device and there is none over a device mask"; return usage(refusal.c_str()); }
    } else if (o.has_matte_ranks || o.has_matte_samples) return usage(o.has_matte_ranks ? "--matte-ranks needs --mattes" : "--matte-samples needs --mattes");
    if (o.demodulate && !o.denoise) return usage("--demodulate-albedo needs --denoise");
    if (o.chain && !o.denoise) return usage("--guide-chain needs --denoise");
    if (o.has_alpha_max && !o.chain) return usage("--guide-alpha-max needs --guide-chain");
    if (o.denoise_bins && o.spectral_bins) return usage("--denoise-spectral-bins cannot be combined with --spectral-bins: it writes the spectral files itself");
    if (o.spectral_bins && o.adaptive >= 0.0f) return usage("--spectral-bins cannot be combined with --adaptive: an adaptive render has no spectral film");
    if (o.spectral_bins && o.denoise) return usage("--spectral-bins cannot be combined with --denoise: the denoiser takes the adaptive path, which has no spectral film");
    if (o.spectral_bins && o.multi) {   // (pt_render_spectral renders on the scene's device, device 0: a mask may name that one alone; 0 = every device of the node)
        if ((o.device_mask & (o.device_mask - 1)) != 0 || (o.device_mask == 0 && pt_device_count() > 1))
            return usage("--spectral-bins cannot be combined with --devices naming more than one GPU: pt_render_multi has no spectral film");
        if (o.device_mask > 1) return usage("--spectral-bins renders on device 0: --devices may name that device alone");
    }
    if (o.resident && !o.denoise) return usage("--denoise-resident needs --denoise");
    if (o.resident && o.multi) return usage("--denoise-resident cannot be combined with --devices: a node render leaves no film one device can filter");
    if (o.resident && o.group_multi) return usage("--denoise-resident cannot be combined with --light-group-devices: a node render leaves no film one device can filter (--denoise-assemble gathers one)");
    if (o.resident && o.spectral_multi) return usage("--denoise-resident cannot be combined with --spectral-devices: a node render leaves no film one device can filter");
    if (o.demodulate_bins && !o.denoise_bins) return usage("--demodulate-bins needs --denoise-spectral-bins");
    if (o.denoise_bins && !o.denoise) return usage("--denoise-spectral-bins needs --denoise");
    if (o.denoise_bins && o.demodulate) return usage("--denoise-spectral-bins cannot be combined with --demodulate-albedo: demodulating the bins needs a per-bin albedo");
    if (o.denoise_bins && o.multi && o.device_mask != 1) return usage("--denoise-spectral-bins renders on device 0: --devices may name that device alone");
    if (o.develop && !o.spectral_bins && !o.denoise_bins) return usage("--develop needs --spectral-bins or --denoise-spectral-bins: it develops their bins");
    if (o.has_develop_filter && !o.develop) return usage("--develop-filter needs --develop");
    if (o.has_develop_subsamples && !o.develop && !o.relamp_groups) return usage("--develop-subsamples needs --develop");
    if (o.spectral_multi && !o.spectral_bins && !o.denoise_bins) return usage("--spectral-devices needs --spectral-bins or --denoise-spectral-bins: it names the devices their spectral film is rendered on");
    if (o.spectral_multi && o.multi) return usage("--spectral-devices cannot be combined with --devices: a spectral render takes its devices from --spectral-devices alone");
    if (o.assemble && o.resident) return usage("--denoise-assemble cannot be combined with --denoise-resident: that flag is the one-device form, this one assembles a node render");
    if (o.assemble && !o.denoise) return usage("--denoise-assemble needs --denoise");
    const bool assemble_groups = o.assemble && o.denoise_groups && o.group_multi;   // (the node group render assembled: the other form of the flag)
    if (o.assemble && !assemble_groups && !o.denoise_bins) return usage("--denoise-assemble needs --denoise-spectral-bins: it assembles the node render of the spectral film");
    if (o.assemble && !assemble_groups && !o.spectral_multi) return usage("--denoise-assemble needs --spectral-devices: it assembles the node render on those devices");
    const bool verbose = o.stdout_log_level == "info" || o.stdout_log_level == "debug" || o.stdout_log_level == "trace";
    const bool warnings = verbose || o.stdout_log_level == "warn";
    if (!o.root.empty()) pt_scene_file_set_root(o.root.c_str());

    pt_config* config = nullptr;
    if (pt_config_load(o.config.c_str(), &config) != PT_OK) {
        fprintf(stderr, "couldn't read config.toml, %s\n", pt_scene_file_last_error());   // main.rs:115-121
        return 1;
    }
    std::string scene_path = o.has_scene ? o.scene : pt_config_scene_file(config);        // main.rs:133
    pt_scene_file* scene_file = nullptr;
    if (pt_scene_file_load(scene_path.c_str(), config, &scene_file) != PT_OK) {
        fprintf(stderr, "failed to construct the scene: %s\n", pt_scene_file_last_error());  // main.rs:139-149
        pt_config_free(config);
        return 1;
    }
    if (warnings) for (uint32_t k = 0; k < pt_scene_file_warning_count(scene_file); ++k) fprintf(stderr, "warning: %s\n", pt_scene_file_warning(scene_file, k));
    const pt_scene_desc* desc = pt_scene_file_desc(scene_file);
    if (verbose) printf("scene %s: %u instances, %u meshes, %zu triangles, %u materials, %u curves\n", scene_path.c_str(), desc->instance_count, desc->mesh_count,
                        desc->index_count / 3, desc->material_count, desc->curve_count);

    // --develop: the response curves and the filter, from the curves library of the scene file (in pt_scene_desc's representation, for pt_spectral_response_matrix)
    std::vector<pt_curve> develop_curves;
    std::vector<float> develop_data;
    int32_t develop_responses[3] = {PT_RESPONSE_CIE_X, PT_RESPONSE_CIE_Y, PT_RESPONSE_CIE_Z}, develop_filter = PT_SPECTRAL_NO_FILTER;
    if (o.develop) {
        std::vector<std::string> names = o.develop_curves;
        if (o.has_develop_filter) names.push_back(o.develop_filter);
        for (size_t k = 0; k < names.size(); ++k) {
            pt_curve c; const float* data = nullptr; uint32_t floats = 0;
            if (pt_scene_file_library_curve(scene_file, names[k].c_str(), &c, &data, &floats) != PT_OK) {
                fprintf(stderr, "error: --develop: %s\n", pt_scene_file_last_error());
                pt_scene_file_free(scene_file);
                pt_config_free(config);
                return 1;
            }
            c.data_offset = (uint32_t)develop_data.size();
            develop_data.insert(develop_data.end(), data, data + floats);
            develop_curves.push_back(c);
            if (k < o.develop_curves.size()) develop_responses[k] = (int32_t)k; else develop_filter = (int32_t)k;
        }
    }

    // --light-groups: a group per emitting instance or per light material in scene order, the environment last when it emits
    std::vector<uint8_t> instance_group(desc->instance_count, 0);
    pt_light_groups_desc gd;
    memset(&gd, 0, sizeof(gd));
    const int group_mode = o.light_groups ? o.light_groups : o.denoise_groups ? o.denoise_groups : o.relamp_groups;
    const char* group_flag = o.light_groups ? "--light-groups" : o.denoise_groups ? "--denoise-light-groups" : "--relamp-groups";
    if (group_mode) {
        std::vector<uint32_t> keys;   // a group's key: the instance (mode 1) or the packed light material (mode 2)
        uint32_t groups = 0;
        for (uint32_t i = 0; i < desc->instance_count; ++i) {
            const pt_instance& in = desc->instances[i];
            uint32_t light = PT_MATERIAL_NONE;   // the instance's first light material
            if (in.material != PT_MATERIAL_NONE) { if (PT_MATERIAL_TAG(in.material) == PT_TAG_LIGHT) light = in.material; }
            else if (in.kind == PT_SHAPE_MESH && in.mesh >= 0 && (uint32_t)in.mesh < desc->mesh_count && desc->meshes[in.mesh].face_material_offset >= 0) {
                const pt_mesh& m = desc->meshes[in.mesh];
                for (uint32_t f = 0; f < m.face_count && light == PT_MATERIAL_NONE; ++f) {
                    const uint32_t id = desc->face_materials[(size_t)m.face_material_offset + f];
                    if (PT_MATERIAL_TAG(id) == PT_TAG_LIGHT) light = id;
                }
            }
            if (light == PT_MATERIAL_NONE) continue;
            const uint32_t key = group_mode == 1 ? i : light;
            uint32_t g = 0;
            while (g < keys.size() && keys[g] != key) ++g;
            if (g == keys.size()) keys.push_back(key);
            if (g < PT_LIGHT_GROUPS_MAX) instance_group[i] = (uint8_t)g;
        }
        groups = (uint32_t)keys.size();
        const bool env_emits = desc->environment.strength != 0.0f;
        gd.environment_group = env_emits ? groups : 0u;
        if (env_emits) ++groups;
        if (groups == 0) groups = 1;
        const char* why = groups > PT_LIGHT_GROUPS_MAX ? "the scene has more than 8 light groups"
                          : (o.has_light_gains && o.light_gains.size() != groups) ? "--light-gains needs one gain per group" : nullptr;
        if (why) {
            fprintf(stderr, "error: %s: %s (%u groups)\n", group_flag, why, groups);
            pt_scene_file_free(scene_file);
            pt_config_free(config);
            return 1;
        }
        gd.group_count = groups; gd.instance_count = desc->instance_count; gd.instance_group = instance_group.data();
        printf("light groups: %u (%s%s)\n", groups, group_mode == 1 ? "one per emitting instance" : "one per light material", env_emits ? ", the environment last" : "");
    }

    if (o.path_passes) {
        printf("path passes: %d (", PT_PATH_PASSES);
        for (int c = 0; c < PT_PATH_PASSES; ++c) printf("%s%s", c ? ", " : "", kPathPassNames[c]);
        printf(")\n");
    }
    const pt_path_passes_desc ppd = {{0u, 0u, 0u, 0u}};

    // --relamp-groups: the curves of pt_light_groups_relamp_matrix — the scene's own, where a group's old curve is, and behind them the new ones from the curves
    // library of the scene file — and per group the old and the new curve
    std::vector<pt_curve> relamp_curves;
    std::vector<float> relamp_data;
    std::vector<int32_t> relamp_old(PT_LIGHT_GROUPS_MAX, PT_RELAMP_KEEP), relamp_new(PT_LIGHT_GROUPS_MAX, PT_RELAMP_KEEP);
    if (o.relamp_groups) {
        const auto refuse = [&](const std::string& why) {
            fprintf(stderr, "error: --relamp-groups: %s\n", why.c_str());
            pt_scene_file_free(scene_file);
            pt_config_free(config);
            return 1;
        };
        if (o.has_relamp_gains && o.relamp_gains.size() != gd.group_count) return refuse("--relamp-gains needs one gain per group (" + std::to_string(gd.group_count) + " groups)");
        relamp_curves.assign(desc->curves, desc->curves + desc->curve_count);
        relamp_data.assign(desc->curve_data, desc->curve_data + desc->curve_data_count);
        const bool env_emits = desc->environment.strength != 0.0f;
        for (const auto& item : o.relamp) {
            const uint32_t g = item.first;
            if (g >= gd.group_count) return refuse("--relamp names group " + std::to_string(g) + ", the scene has " + std::to_string(gd.group_count) + " groups");
            // the emission curve the group's emitters share: every light material of its instances, and the environment's curve when it is the environment's group
            int32_t old = -1;
            bool mixed = false, any = false;
            const auto emitter = [&](int32_t curve) { mixed = mixed || (any && curve != old); old = curve; any = true; };
            if (env_emits && gd.environment_group == g) {
                if (desc->environment.kind == PT_ENV_HDR)
                    return refuse("--relamp names group " + std::to_string(g) + ", the environment, which an HDR texture lights: it has no single emission curve to replace");
                emitter(desc->environment.curve);
            }
            for (uint32_t i = 0; i < desc->instance_count; ++i) {
                if (instance_group[i] != g) continue;
                const pt_instance& in = desc->instances[i];
                const auto light = [&](uint32_t id) { if (PT_MATERIAL_TAG(id) == PT_TAG_LIGHT && PT_MATERIAL_INDEX(id) < desc->material_count) emitter(desc->materials[PT_MATERIAL_INDEX(id)].curve_emit); };
                if (in.material != PT_MATERIAL_NONE) light(in.material);
                else if (in.kind == PT_SHAPE_MESH && in.mesh >= 0 && (uint32_t)in.mesh < desc->mesh_count && desc->meshes[in.mesh].face_material_offset >= 0) {
                    const pt_mesh& m = desc->meshes[in.mesh];
                    for (uint32_t f = 0; f < m.face_count; ++f) light(desc->face_materials[(size_t)m.face_material_offset + f]);
                }
            }
            if (!any) return refuse("--relamp names group " + std::to_string(g) + ", which holds no emitter");
            if (mixed) return refuse("--relamp names group " + std::to_string(g) + ", whose emitters have different emission curves: it has no single curve to replace");
            pt_curve c; const float* data = nullptr; uint32_t floats = 0;
            if (pt_scene_file_library_curve(scene_file, item.second.c_str(), &c, &data, &floats) != PT_OK) return refuse(std::string("--relamp: ") + pt_scene_file_last_error());
            c.data_offset = (uint32_t)relamp_data.size();
            relamp_data.insert(relamp_data.end(), data, data + floats);
            relamp_old[g] = old; relamp_new[g] = (int32_t)relamp_curves.size();
            relamp_curves.push_back(c);
        }
    }

    // --denoise: what the adaptive path refuses is refused here, with its message, before anything is rendered or written
    if (o.denoise && !o.dry_run) {
        uint32_t tw = 0, th = 0;
        const bool naive = pt_config_renderer(config, &tw, &th) == PT_RENDERER_NAIVE;
        for (uint32_t i = 0; i < pt_config_render_settings_count(config); ++i) {
            pt_render_settings rs; pt_render_desc rd;
            pt_config_render_settings(config, i, &rs);
            if (pt_config_render_desc(config, i, o.seed, &rd) != PT_OK) continue;   // (skipped below as well)
            const bool range = o.adaptive >= 0.0f && !naive && rs.max_samples >= 0 && (uint32_t)rs.max_samples > rd.spp;   // (--adaptive rounds a range up itself)
            const char* why = naive ? "adaptive sampling needs phases of 10 samples (phase_samples 0 or 10)"
                                    : ((!range && rd.spp % 10u != 0u) ? "spp, step and max_samples must be multiples of 10" : nullptr);
            if (why) {
                fprintf(stderr, "error: --denoise: render settings %u (%s, min_samples %u) cannot take the adaptive path the statistics come from: %s\n", i,
                        naive ? "Naive renderer" : "Tiled renderer", rd.spp, why);
                pt_scene_file_free(scene_file);
                pt_config_free(config);
                return 1;
            }
        }
    }

    printf("constructing renderer\n");
    mkdir(o.output_dir.c_str(), 0777);                                                     // main.rs:155-158
    int rc = 0;
    if (!o.dry_run) {
        pt_scene* scene = nullptr;
        if (pt_scene_create(desc, &scene) != PT_OK) { fprintf(stderr, "pt_scene_create: %s\n", pt_last_error()); rc = 1; }
        const uint32_t n = pt_config_render_settings_count(config);
        for (uint32_t i = 0; rc == 0 && i < n; ++i) {
            pt_render_settings rs; pt_render_desc rd; pt_output_desc od;
            pt_config_render_settings(config, i, &rs);
            if (pt_config_render_desc(config, i, o.seed, &rd) != PT_OK) {
                // the reference skips render settings whose integrator it cannot construct (src/renderer/tiled.rs:560-566)
                fprintf(stderr, "skipping render settings %u: %s\n", i, pt_scene_file_last_error());
                continue;
            }
            if (o.hero) rd.hero_wavelengths = o.hero;   // engine extension (not in the reference's files): 4 wavelengths per path
            std::vector<float> film((size_t)rd.width * rd.height * 4);
            pt_profile prof;
            // --adaptive: min_samples .. max_samples per pixel (pt_render_adaptive) where the setting gives a range and the renderer sums in phases of 10
            bool adaptive = o.adaptive >= 0.0f;
            pt_adaptive_desc ad = {0u, 0u, o.adaptive, 0.0f};
            if (adaptive) {
                uint32_t tw = 0, th = 0;
                if (pt_config_renderer(config, &tw, &th) == PT_RENDERER_NAIVE) {
                    if (warnings) fprintf(stderr, "warning: --adaptive: render settings %u use the Naive renderer; rendering %u spp everywhere\n", i, rd.spp);
                    adaptive = false;
                } else if (rs.max_samples < 0 || (uint32_t)rs.max_samples <= rd.spp) {
                    if (warnings) fprintf(stderr, "warning: --adaptive: render settings %u have no max_samples > min_samples; rendering %u spp everywhere\n", i, rd.spp);
                    adaptive = false;
                } else {
                    const uint32_t lo = (rd.spp + 9u) / 10u * 10u, hi = ((uint32_t)rs.max_samples + 9u) / 10u * 10u;
                    if ((lo != rd.spp || hi != (uint32_t)rs.max_samples) && warnings)
                        fprintf(stderr, "warning: --adaptive: samples %u..%d rounded up to %u..%u (multiples of 10)\n", rd.spp, rs.max_samples, lo, hi);
                    rd.spp = lo; ad.max_samples = hi;
                }
            }
            const bool with_counts = adaptive || o.denoise;
            std::vector<uint32_t> counts(with_counts ? (size_t)rd.width * rd.height : 0);
            std::vector<double> stats(o.denoise ? (size_t)rd.width * rd.height * 2 : 0);
            std::vector<float> spectral((size_t)o.denoise_bins * rd.width * rd.height);   // (--spectral-bins sizes it below)
            std::vector<float> group_films;   // (--light-groups sizes it below)
            std::vector<float> group_bins;    // (--relamp-groups sizes it below)
            const pt_spectral_desc dsd = {o.denoise_bins, {0u, 0u, 0u}};
            const char* adaptive_entry = o.denoise_bins ? (o.spectral_multi ? "pt_render_adaptive_spectral_multi" : "pt_render_adaptive_spectral")
                                         : o.denoise_groups ? (o.group_multi ? "pt_render_adaptive_light_groups_multi" : "pt_render_adaptive_light_groups")
                                         : o.denoise_passes ? "pt_render_adaptive_path_passes" : o.multi ? "pt_render_adaptive_multi" : "pt_render_adaptive";
            if (o.denoise_groups) group_films.resize((size_t)gd.group_count * rd.width * rd.height * 4);
            if (o.path_passes) group_films.resize((size_t)PT_PATH_PASSES * rd.width * rd.height * 4);
            // --denoise-path-passes: the adaptive pass render — film, counts and statistics are pt_render_adaptive's bit for bit
            const auto adaptive_passes = [&] { return pt_render_adaptive_path_passes(scene, &rd, &ad, &ppd, film.data(), counts.data(), stats.data(), group_films.data(), &prof); };
            // --denoise-light-groups: the adaptive group render — film, counts and statistics are pt_render_adaptive's bit for bit
            // (--light-group-devices: on the devices of the mask)
            const auto adaptive_groups = [&] {
                return o.group_multi ? pt_render_adaptive_light_groups_multi(scene, &rd, &ad, &gd, o.group_device_mask, film.data(), counts.data(), stats.data(), group_films.data(), &prof)
                                     : pt_render_adaptive_light_groups(scene, &rd, &ad, &gd, film.data(), counts.data(), stats.data(), group_films.data(), &prof);
            };
            // --denoise-spectral-bins: the adaptive spectral render, on one device or (--spectral-devices) on the devices of the mask
            const auto adaptive_spectral = [&](double* st_out) {
                return o.spectral_multi ? pt_render_adaptive_spectral_multi(scene, &rd, &ad, &dsd, o.spectral_device_mask, film.data(), counts.data(), st_out, spectral.data(), &prof)
                                        : pt_render_adaptive_spectral(scene, &rd, &ad, &dsd, film.data(), counts.data(), st_out, spectral.data(), &prof);
            };
            uint64_t samples = (uint64_t)rd.width * rd.height * rd.spp;
            if (!adaptive && o.denoise) {
                // a fixed count through the adaptive path (max_samples = min_samples, one round): pt_render's film bit for bit, and the statistics
                printf("rendering %ux%u, %u spp, max_bounces %u, light_samples %u\n", rd.width, rd.height, rd.spp, rd.max_bounces, rd.light_samples);
                ad.max_samples = rd.spp; ad.rel_error = 0.0f;
                const pt_status st = o.denoise_bins ? adaptive_spectral(stats.data())
                                     : o.denoise_groups ? adaptive_groups()
                                     : o.denoise_passes ? adaptive_passes()
                                     : o.multi      ? pt_render_adaptive_multi(scene, &rd, &ad, o.device_mask, film.data(), counts.data(), stats.data(), &prof)
                                                    : pt_render_adaptive(scene, &rd, &ad, film.data(), counts.data(), stats.data(), &prof);
                if (st != PT_OK) { fprintf(stderr, "%s: %s\n", adaptive_entry, pt_last_error()); rc = 1; break; }
            } else if (adaptive) {
                printf("rendering %ux%u, %u..%u spp (adaptive, relative error %g), max_bounces %u, light_samples %u\n", rd.width, rd.height, rd.spp, ad.max_samples,
                       (double)ad.rel_error, rd.max_bounces, rd.light_samples);
                const pt_status st = o.denoise_bins ? adaptive_spectral(stats.data())
                                     : o.denoise_groups ? adaptive_groups()
                                     : o.denoise_passes ? adaptive_passes()
                                     : o.multi      ? pt_render_adaptive_multi(scene, &rd, &ad, o.device_mask, film.data(), counts.data(), o.denoise ? stats.data() : nullptr, &prof)
                                                    : pt_render_adaptive(scene, &rd, &ad, film.data(), counts.data(), o.denoise ? stats.data() : nullptr, &prof);
                if (st != PT_OK) { fprintf(stderr, "%s: %s\n", adaptive_entry, pt_last_error()); rc = 1; break; }
                uint32_t lo = 0xffffffffu, hi = 0;
                samples = 0;
                for (uint32_t c : counts) { samples += c; lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
                printf("adaptive: %.2f samples per pixel on average, min %u, max %u, %llu rounds\n", (double)samples / (double)counts.size(), lo, hi,
                       (unsigned long long)prof.kernel_launches[5]);
            } else if (o.spectral_bins) {
                printf("rendering %ux%u, %u spp, max_bounces %u, light_samples %u\n", rd.width, rd.height, rd.spp, rd.max_bounces, rd.light_samples);
                spectral.resize((size_t)o.spectral_bins * rd.width * rd.height);
                const pt_spectral_desc sd = {o.spectral_bins, {0u, 0u, 0u}};
                const pt_status st = o.spectral_multi ? pt_render_spectral_multi(scene, &rd, &sd, o.spectral_device_mask, film.data(), spectral.data(), &prof)
                                                      : pt_render_spectral(scene, &rd, &sd, film.data(), spectral.data(), &prof);
                if (st != PT_OK) { fprintf(stderr, "%s: %s\n", o.spectral_multi ? "pt_render_spectral_multi" : "pt_render_spectral", pt_last_error()); rc = 1; break; }
            } else if (o.relamp_groups) {
                printf("rendering %ux%u, %u spp, max_bounces %u, light_samples %u, %u light groups of %u bins\n", rd.width, rd.height, rd.spp, rd.max_bounces, rd.light_samples,
                       gd.group_count, o.relamp_bins);
                group_bins.resize((size_t)gd.group_count * o.relamp_bins * rd.width * rd.height);
                const pt_spectral_desc sd = {o.relamp_bins, {0u, 0u, 0u}};
                if (pt_render_light_groups_spectral(scene, &rd, &gd, &sd, film.data(), nullptr, nullptr, group_bins.data(), &prof) != PT_OK) {
                    fprintf(stderr, "pt_render_light_groups_spectral: %s\n", pt_last_error()); rc = 1; break;
                }
            } else if (o.path_passes) {
                printf("rendering %ux%u, %u spp, max_bounces %u, light_samples %u, %d path passes\n", rd.width, rd.height, rd.spp, rd.max_bounces, rd.light_samples, PT_PATH_PASSES);
                if (pt_render_path_passes(scene, &rd, &ppd, film.data(), group_films.data(), &prof) != PT_OK) { fprintf(stderr, "pt_render_path_passes: %s\n", pt_last_error()); rc = 1; break; }
            } else if (o.light_groups) {
                printf("rendering %ux%u, %u spp, max_bounces %u, light_samples %u, %u light groups\n", rd.width, rd.height, rd.spp, rd.max_bounces, rd.light_samples, gd.group_count);
                group_films.resize((size_t)gd.group_count * rd.width * rd.height * 4);
                const pt_status st = o.group_multi ? pt_render_light_groups_multi(scene, &rd, &gd, o.group_device_mask, film.data(), group_films.data(), &prof)
                                                   : pt_render_light_groups(scene, &rd, &gd, film.data(), group_films.data(), &prof);
                if (st != PT_OK) { fprintf(stderr, "%s: %s\n", o.group_multi ? "pt_render_light_groups_multi" : "pt_render_light_groups", pt_last_error()); rc = 1; break; }
            } else {
                printf("rendering %ux%u, %u spp, max_bounces %u, light_samples %u\n", rd.width, rd.height, rd.spp, rd.max_bounces, rd.light_samples);
                const pt_status st = o.multi ? pt_render_multi(scene, &rd, o.device_mask, film.data(), &prof) : pt_render(scene, &rd, film.data(), &prof);
                if (st != PT_OK) { fprintf(stderr, "%s: %s\n", o.multi ? "pt_render_multi" : "pt_render", pt_last_error()); rc = 1; break; }
            }
            // Profile::pretty_print (src/profile.rs:20-34)
            const double total = (double)(prof.camera_rays + prof.bounce_rays + prof.shadow_rays + prof.light_rays);
            printf("took %.3fs\n", prof.seconds);
            printf("%llu camera rays, %llu bounce rays, %llu shadow rays, %llu light rays, %llu environment hits\n", (unsigned long long)prof.camera_rays,
                   (unsigned long long)prof.bounce_rays, (unsigned long long)prof.shadow_rays, (unsigned long long)prof.light_rays, (unsigned long long)prof.env_hits);
            printf("%.1f rays per second, %.3f Msamples/s\n", total / prof.seconds, (double)samples / prof.seconds * 1e-6);
            pt_config_output_desc(config, i, 1.0f, &od);
            std::vector<uint8_t> rgba((size_t)rd.width * rd.height * 4);
            std::vector<float> linear((size_t)rd.width * rd.height * 3);
            if (pt_output_film(&od, film.data(), rgba.data(), linear.data()) != PT_OK) { fprintf(stderr, "pt_output_film: %s\n", pt_last_error()); rc = 1; break; }
            const std::string base = o.output_dir + "/" + (rs.filename ? rs.filename : "beauty");  // src/renderer/mod.rs:27-31
            if (pt_write_exr((base + ".exr").c_str(), rd.width, rd.height, linear.data(), od.colorspace) != PT_OK ||
                pt_write_png((base + ".png").c_str(), rd.width, rd.height, rgba.data(), od.colorspace) != PT_OK) {
                fprintf(stderr, "failed to write files: %s\n", pt_last_error()); rc = 1; break;  // the reference panics here (mod.rs:45-48)
            }
            if (o.write_film && !write_npy(base + ".npy", film.data(), rd.height, rd.width)) { fprintf(stderr, "failed to write %s.npy\n", base.c_str()); rc = 1; break; }
            printf("wrote %s.exr and %s.png\n", base.c_str(), base.c_str());
            // --mattes: the ranked ids of this setting's frame (pt_render_mattes, beside the render: no file above changes) as a Cryptomatte file with the
            // setting's linear RGB — instances named instance<i>, materials by their names in the scene file's library
            if (o.mattes) {
                const size_t np = (size_t)rd.width * rd.height;
                const pt_matte_desc md = {o.matte_samples ? o.matte_samples : (rs.min_samples < 65535u ? rs.min_samples : 65535u), o.matte_ranks,
                                          o.mattes == 2 ? (uint32_t)PT_MATTE_KEY_MATERIAL : (uint32_t)PT_MATTE_KEY_INSTANCE, {0u}};
                std::vector<uint32_t> m_keys(md.ranks * np), m_overflow(np), named;
                std::vector<float> m_coverage(md.ranks * np);
                if (pt_render_mattes(scene, &rd, &md, m_keys.data(), m_coverage.data(), m_overflow.data()) != PT_OK) { fprintf(stderr, "pt_render_mattes: %s\n", pt_last_error()); rc = 1; break; }
                std::vector<std::string> names;
                for (uint32_t key : m_keys) {
                    if (key == PT_MATTE_SKY || key == PT_MATTE_NONE) continue;
                    bool seen = false;
                    for (uint32_t k : named) seen = seen || k == key;
                    if (seen) continue;
                    const char* material = o.mattes == 2 ? pt_scene_file_material_name(scene_file, key) : nullptr;
                    named.push_back(key);
                    names.push_back(o.mattes == 1 ? "instance" + std::to_string(key) : material ? std::string(material) : "key" + std::to_string(key));
                }
                std::vector<const char*> name_ptrs;
                for (const std::string& s : names) name_ptrs.push_back(s.c_str());
                uint64_t dropped = 0;
                for (uint32_t c : m_overflow) dropped += c;
                const std::string crypto = base + "_crypto.exr";
                if (pt_write_exr_cryptomatte(crypto.c_str(), rd.width, rd.height, md.ranks, m_keys.data(), m_coverage.data(), o.mattes == 2 ? "CryptoMaterial" : "CryptoObject",
                                             (uint32_t)named.size(), named.data(), name_ptrs.data(), linear.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "failed to write %s: %s\n", crypto.c_str(), pt_last_error()); rc = 1; break;
                }
                printf("wrote %s (%u ranks of %u samples, %zu names, %llu samples beyond the ranks)\n", crypto.c_str(), md.ranks, md.samples, names.size(), (unsigned long long)dropped);
            }
            // --light-groups, --denoise-light-groups: every group's film, and with --light-gains the resident mix, through this setting's film output (buffers of
            // their own).  `stem`: base, or base + "_denoised" for the films of the joint filter, which are then mixed where that left them.
            // (host_mix: the films were filtered over host arrays and are mixed from there, pt_light_groups_mix)
            const auto write_groups = [&](const std::string& stem, const std::vector<float>& films, bool denoised, bool host_mix = false) {
                const size_t np = (size_t)rd.width * rd.height;
                std::vector<float> g_linear(3 * np), relit(4 * np), matrices;
                std::vector<uint8_t> g_rgba(4 * np);
                bool ok = true;
                for (uint32_t g = 0; ok && g < gd.group_count; ++g) {
                    const std::string name = stem + "_light" + std::to_string(g);
                    ok = pt_output_film(&od, films.data() + 4 * np * g, g_rgba.data(), g_linear.data()) == PT_OK &&
                         pt_write_exr((name + ".exr").c_str(), rd.width, rd.height, g_linear.data(), od.colorspace) == PT_OK;
                    if (ok) printf("wrote %s.exr\n", name.c_str());
                }
                if (ok && o.has_light_gains) {
                    for (float gain : o.light_gains) for (int k = 0; k < 9; ++k) matrices.push_back(k % 4 == 0 ? gain : 0.0f);
                    const std::string name = stem + "_relit";
                    ok = (host_mix ? pt_light_groups_mix(rd.width, rd.height, gd.group_count, films.data(), matrices.data(), relit.data())
                          : denoised ? pt_light_groups_mix_resident_denoised(scene, matrices.data(), relit.data()) : pt_light_groups_mix_resident(scene, matrices.data(), relit.data())) == PT_OK &&
                         pt_output_film(&od, relit.data(), g_rgba.data(), g_linear.data()) == PT_OK &&
                         pt_write_exr((name + ".exr").c_str(), rd.width, rd.height, g_linear.data(), od.colorspace) == PT_OK &&
                         pt_write_png((name + ".png").c_str(), rd.width, rd.height, g_rgba.data(), od.colorspace) == PT_OK;
                    if (ok) printf("wrote %s.exr and %s.png (relit from %u light groups)\n", name.c_str(), name.c_str(), gd.group_count);
                }
                if (!ok) fprintf(stderr, "%s: %s\n", group_flag, pt_last_error());
                return ok;
            };
            if (group_mode && !o.relamp_groups && !write_groups(base, group_films, false)) { rc = 1; break; }
            // --path-passes: every class's film through this setting's film output (buffers of their own).  `stem`: base, or base + "_denoised"
            const auto write_passes = [&](const std::string& stem, const std::vector<float>& films) {
                const size_t np = (size_t)rd.width * rd.height;
                std::vector<float> p_linear(3 * np);
                std::vector<uint8_t> p_rgba(4 * np);
                bool ok = true;
                for (int c = 0; ok && c < PT_PATH_PASSES; ++c) {
                    const std::string name = stem + "_pass_" + kPathPassNames[c];
                    ok = pt_output_film(&od, films.data() + 4 * np * c, p_rgba.data(), p_linear.data()) == PT_OK &&
                         pt_write_exr((name + ".exr").c_str(), rd.width, rd.height, p_linear.data(), od.colorspace) == PT_OK;
                    if (ok) printf("wrote %s.exr\n", name.c_str());
                }
                if (!ok) fprintf(stderr, "--path-passes: %s\n", pt_last_error());
                return ok;
            };
            if (o.path_passes && !write_passes(base, group_films)) { rc = 1; break; }
            // --relamp-groups: every group's bins in the units of the EXR payload, and the re-lamped picture — the colour-matching development of the group bins by
            // the re-lamp matrix, where the render left them on the device — through this setting's film output (buffers of its own)
            if (o.relamp_groups) {
                const size_t np = (size_t)rd.width * rd.height, plane = (size_t)o.relamp_bins * np;
                const pt_spectral_desc sd = {o.relamp_bins, {0u, 0u, 0u}};
                std::vector<float> centres(o.relamp_bins), scaled(plane), matrix((size_t)3 * gd.group_count * o.relamp_bins), planes(3 * np), packed(4 * np), r_linear(3 * np);
                std::vector<uint8_t> r_rgba(4 * np);
                bool ok = pt_spectral_bin_centres(&rd, &sd, centres.data()) == PT_OK;
                for (uint32_t g = 0; ok && g < gd.group_count; ++g) {
                    const std::string name = base + "_light" + std::to_string(g) + "_spectral";
                    for (size_t k = 0; k < plane; ++k) scaled[k] = group_bins[plane * g + k] * od.factor;
                    ok = pt_write_exr_spectral((name + ".exr").c_str(), rd.width, rd.height, o.relamp_bins, centres.data(), scaled.data(), nullptr, od.colorspace) == PT_OK;
                    if (ok) printf("wrote %s.exr (%u bins)\n", name.c_str(), o.relamp_bins);
                }
                const int32_t cie[3] = {PT_RESPONSE_CIE_X, PT_RESPONSE_CIE_Y, PT_RESPONSE_CIE_Z};
                ok = ok && pt_light_groups_relamp_matrix(&rd, &sd, relamp_curves.data(), (uint32_t)relamp_curves.size(), relamp_data.data(), (uint32_t)relamp_data.size(), 3, cie,
                                                         PT_SPECTRAL_NO_FILTER, o.develop_subsamples, gd.group_count, relamp_old.data(), relamp_new.data(),
                                                         o.has_relamp_gains ? o.relamp_gains.data() : nullptr, matrix.data()) == PT_OK &&
                     pt_light_groups_relamp_resident(scene, 3, matrix.data(), planes.data()) == PT_OK;
                if (ok) {
                    for (size_t p = 0; p < np; ++p) { packed[4 * p] = planes[p]; packed[4 * p + 1] = planes[np + p]; packed[4 * p + 2] = planes[2 * np + p]; packed[4 * p + 3] = 0.0f; }
                    const std::string name = base + "_relamped";
                    ok = pt_output_film(&od, packed.data(), r_rgba.data(), r_linear.data()) == PT_OK &&
                         pt_write_exr((name + ".exr").c_str(), rd.width, rd.height, r_linear.data(), od.colorspace) == PT_OK &&
                         pt_write_png((name + ".png").c_str(), rd.width, rd.height, r_rgba.data(), od.colorspace) == PT_OK;
                    if (ok) printf("wrote %s.exr and %s.png (re-lamped from %u light groups of %u bins)\n", name.c_str(), name.c_str(), gd.group_count, o.relamp_bins);
                }
                if (!ok) { fprintf(stderr, "--relamp-groups: %s\n", pt_last_error()); rc = 1; break; }
            }
            // the bins in the units of the EXR payload: the same factor, applied here in place, one multiply per value
            const uint32_t file_bins = o.spectral_bins ? o.spectral_bins : o.denoise_bins;
            const auto write_spectral = [&](const std::string& name, std::vector<float>& scaled) {
                const pt_spectral_desc sd = {file_bins, {0u, 0u, 0u}};
                std::vector<float> centres(file_bins);
                for (float& v : scaled) v *= od.factor;
                if (pt_spectral_bin_centres(&rd, &sd, centres.data()) != PT_OK ||
                    pt_write_exr_spectral((name + ".exr").c_str(), rd.width, rd.height, file_bins, centres.data(), scaled.data(), linear.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "%s: %s\n", o.spectral_bins ? "--spectral-bins" : "--denoise-spectral-bins", pt_last_error());
                    return false;
                }
                printf("wrote %s.exr (%u bins)\n", name.c_str(), file_bins);
                return true;
            };
            if (o.denoise_bins) {   // (a copy: the filter below takes the bins as rendered)
                std::vector<float> noisy(spectral);
                if (!write_spectral(base + "_spectral", noisy)) { rc = 1; break; }
            } else if (!spectral.empty() && !write_spectral(base + "_spectral", spectral)) { rc = 1; break; }
            // --develop: three planes from the bins — the scene's resident ones (bins == nullptr; `denoised`: the resident denoised ones) or a host array as rendered
            // or filtered, before the factor —, packed as an XYZW film with W = 0, through this setting's film output (buffers of its own: `linear` still serves
            // the spectral files)
            const auto develop = [&](const std::string& name, const float* bins, bool denoised = false) {
                const pt_spectral_desc sd = {file_bins, {0u, 0u, 0u}};
                const size_t np = (size_t)rd.width * rd.height;
                std::vector<float> matrix((size_t)3 * file_bins), planes(3 * np), packed(4 * np), dev_linear(3 * np);
                std::vector<uint8_t> dev_rgba(4 * np);
                pt_status st = pt_spectral_response_matrix(&rd, &sd, develop_curves.data(), (uint32_t)develop_curves.size(), develop_data.data(), (uint32_t)develop_data.size(),
                                                           3, develop_responses, develop_filter, o.develop_subsamples, matrix.data());
                if (st == PT_OK) st = bins       ? pt_spectral_project(rd.width, rd.height, file_bins, 3, matrix.data(), bins, planes.data())
                                      : denoised ? pt_spectral_project_resident_denoised(scene, 3, matrix.data(), planes.data())
                                                 : pt_spectral_project_resident(scene, 3, matrix.data(), planes.data());
                if (st != PT_OK) { fprintf(stderr, "--develop: %s\n", pt_last_error()); return false; }
                for (size_t p = 0; p < np; ++p) { packed[4 * p] = planes[p]; packed[4 * p + 1] = planes[np + p]; packed[4 * p + 2] = planes[2 * np + p]; packed[4 * p + 3] = 0.0f; }
                if (pt_output_film(&od, packed.data(), dev_rgba.data(), dev_linear.data()) != PT_OK ||
                    pt_write_exr((name + ".exr").c_str(), rd.width, rd.height, dev_linear.data(), od.colorspace) != PT_OK ||
                    pt_write_png((name + ".png").c_str(), rd.width, rd.height, dev_rgba.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "--develop: %s\n", pt_last_error());
                    return false;
                }
                printf("wrote %s.exr and %s.png (developed from %u bins)\n", name.c_str(), name.c_str(), file_bins);
                return true;
            };
            // (a node render leaves its bins resident too, with either flag: they are developed on the devices)
            if (o.develop && !develop(base + "_developed", o.denoise_bins && !o.spectral_multi && !o.resident ? spectral.data() : nullptr)) { rc = 1; break; }
            if (o.denoise && o.assemble) {
                // the node render left its pieces on the devices: one film on the scene's device from them, unless the mask came down to that device alone and
                // the render left the film resident itself
                struct pt_resident_info now;
                pt_status ast = pt_resident_info(scene, &now);
                if (ast == PT_OK && !(now.parts & PT_RESIDENT_FILM)) ast = pt_resident_assemble(scene, 0u);
                if (ast != PT_OK) { fprintf(stderr, "--denoise-assemble: %s\n", pt_last_error()); rc = 1; break; }
            }
            // (a node group render without --denoise-assemble left no film one device can filter, unless the mask came down to the scene's device alone)
            bool groups_on_host = false;
            if (o.denoise && o.denoise_groups && o.group_multi && !o.assemble) {
                struct pt_resident_info now;
                if (pt_resident_info(scene, &now) != PT_OK) { fprintf(stderr, "--light-group-devices: %s\n", pt_last_error()); rc = 1; break; }
                groups_on_host = !(now.parts & PT_RESIDENT_FILM);
            }
            if (o.denoise && o.denoise_groups && groups_on_host) {
                // guides and the joint filter over host arrays, on the first device of the mask: the files of the resident route, byte for byte
                const size_t np = (size_t)rd.width * rd.height;
                std::vector<float> guides(4 * np), albedo(o.demodulate ? 4 * np : 0), clean(4 * np), clean_groups(4 * np * gd.group_count);
                pt_denoise_desc dd;
                memset(&dd, 0, sizeof(dd));
                dd.width = rd.width; dd.height = rd.height;
                if (o.group_device_mask) while (!((o.group_device_mask >> dd.device) & 1u)) ++dd.device;
                pt_guide_chain_desc cd;
                memset(&cd, 0, sizeof(cd));
                cd.max_chain = o.max_chain; cd.alpha_max = o.alpha_max;
                pt_status dst = o.chain ? pt_render_guides_chain(scene, &rd, o.guide_samples, &cd, guides.data(), o.demodulate ? albedo.data() : nullptr)
                                : o.demodulate ? pt_render_guides_albedo(scene, &rd, o.guide_samples, guides.data(), albedo.data())
                                               : pt_render_guides(scene, &rd, o.guide_samples, guides.data());
                if (dst == PT_OK) dst = pt_denoise_light_groups(&dd, gd.group_count, film.data(), counts.data(), stats.data(), guides.data(), o.demodulate ? albedo.data() : nullptr,
                                                                group_films.data(), clean.data(), nullptr, clean_groups.data());
                if (dst != PT_OK) { fprintf(stderr, "--denoise-light-groups: %s\n", pt_last_error()); rc = 1; break; }
                if (pt_output_film(&od, clean.data(), rgba.data(), linear.data()) != PT_OK) { fprintf(stderr, "pt_output_film: %s\n", pt_last_error()); rc = 1; break; }
                const std::string dbase = base + "_denoised";
                if (pt_write_exr((dbase + ".exr").c_str(), rd.width, rd.height, linear.data(), od.colorspace) != PT_OK ||
                    pt_write_png((dbase + ".png").c_str(), rd.width, rd.height, rgba.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "failed to write files: %s\n", pt_last_error()); rc = 1; break;
                }
                if (o.write_film && !write_npy(dbase + ".npy", clean.data(), rd.height, rd.width)) { fprintf(stderr, "failed to write %s.npy\n", dbase.c_str()); rc = 1; break; }
                printf("wrote %s.exr and %s.png\n", dbase.c_str(), dbase.c_str());
                if (!write_groups(dbase, clean_groups, true, true)) { rc = 1; break; }
            } else if (o.denoise && (o.denoise_groups || o.denoise_passes)) {
                // the render left the film, its statistics and the group films on the device, paired: the guides stay there too, and the joint filter runs on all of
                // it (with or without --denoise-resident: this is the only route, and its files are those of either)
                const size_t np = (size_t)rd.width * rd.height;
                // (--denoise-path-passes: the pass films are the resident group films of this route)
                const char* const flag = o.denoise_passes ? "--denoise-path-passes" : "--denoise-light-groups";
                std::vector<float> clean(4 * np), clean_groups(4 * np * (o.denoise_passes ? (uint32_t)PT_PATH_PASSES : gd.group_count));
                pt_guide_chain_desc cd;
                memset(&cd, 0, sizeof(cd));
                cd.max_chain = o.max_chain; cd.alpha_max = o.alpha_max;
                pt_resident_denoise_desc dd;
                memset(&dd, 0, sizeof(dd));
                pt_status dst = pt_resident_guides(scene, &rd, o.guide_samples, o.chain ? &cd : nullptr, o.demodulate ? PT_RESIDENT_ALBEDO : 0u);
                if (dst == PT_OK) dst = pt_denoise_light_groups_resident(scene, &dd, clean.data(), nullptr, clean_groups.data());
                if (dst != PT_OK) { fprintf(stderr, "%s: %s\n", flag, pt_last_error()); rc = 1; break; }
                if (pt_output_film(&od, clean.data(), rgba.data(), linear.data()) != PT_OK) { fprintf(stderr, "pt_output_film: %s\n", pt_last_error()); rc = 1; break; }
                const std::string dbase = base + "_denoised";
                if (pt_write_exr((dbase + ".exr").c_str(), rd.width, rd.height, linear.data(), od.colorspace) != PT_OK ||
                    pt_write_png((dbase + ".png").c_str(), rd.width, rd.height, rgba.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "failed to write files: %s\n", pt_last_error()); rc = 1; break;
                }
                if (o.write_film && !write_npy(dbase + ".npy", clean.data(), rd.height, rd.width)) { fprintf(stderr, "failed to write %s.npy\n", dbase.c_str()); rc = 1; break; }
                printf("wrote %s.exr and %s.png\n", dbase.c_str(), dbase.c_str());
                if (!(o.denoise_passes ? write_passes(dbase, clean_groups) : write_groups(dbase, clean_groups, true))) { rc = 1; break; }
            } else if (o.denoise && (o.resident || o.assemble)) {
                // the render left film, counts, statistics and bins on the device: the guides stay there too, and the filter runs on all of it
                std::vector<float> clean((size_t)rd.width * rd.height * 4), clean_spectral(spectral.size());
                pt_guide_chain_desc cd;
                memset(&cd, 0, sizeof(cd));
                cd.max_chain = o.max_chain; cd.alpha_max = o.alpha_max;
                pt_resident_denoise_desc dd;
                memset(&dd, 0, sizeof(dd));
                const uint32_t parts = o.demodulate_bins ? (PT_RESIDENT_ALBEDO | PT_RESIDENT_BIN_ALBEDO) : o.demodulate ? PT_RESIDENT_ALBEDO : 0u;
                pt_status dst = pt_resident_guides(scene, &rd, o.guide_samples, o.chain ? &cd : nullptr, parts);
                if (dst == PT_OK) dst = pt_denoise_resident(scene, &dd, clean.data(), nullptr, o.denoise_bins ? clean_spectral.data() : nullptr);
                if (dst != PT_OK) { fprintf(stderr, "%s: %s\n", o.assemble ? "--denoise-assemble" : "--denoise-resident", pt_last_error()); rc = 1; break; }
                if (pt_output_film(&od, clean.data(), rgba.data(), linear.data()) != PT_OK) { fprintf(stderr, "pt_output_film: %s\n", pt_last_error()); rc = 1; break; }
                const std::string dbase = base + "_denoised";
                if (pt_write_exr((dbase + ".exr").c_str(), rd.width, rd.height, linear.data(), od.colorspace) != PT_OK ||
                    pt_write_png((dbase + ".png").c_str(), rd.width, rd.height, rgba.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "failed to write files: %s\n", pt_last_error()); rc = 1; break;
                }
                if (o.write_film && !write_npy(dbase + ".npy", clean.data(), rd.height, rd.width)) { fprintf(stderr, "failed to write %s.npy\n", dbase.c_str()); rc = 1; break; }
                printf("wrote %s.exr and %s.png\n", dbase.c_str(), dbase.c_str());
                if (o.develop && o.denoise_bins && !develop(dbase + "_developed", nullptr, true)) { rc = 1; break; }
                if (o.denoise_bins && !write_spectral(dbase + "_spectral", clean_spectral)) { rc = 1; break; }
            } else if (o.denoise) {
                std::vector<float> guides((size_t)rd.width * rd.height * 4), clean((size_t)rd.width * rd.height * 4);
                pt_denoise_desc dd;
                memset(&dd, 0, sizeof(dd));
                dd.width = rd.width; dd.height = rd.height;
                if (o.multi && o.device_mask) while (!((o.device_mask >> dd.device) & 1u)) ++dd.device;   // (the first device of the mask: where the gather left the film)
                if (o.spectral_multi && o.spectral_device_mask) while (!((o.spectral_device_mask >> dd.device) & 1u)) ++dd.device;
                std::vector<float> albedo(o.demodulate || o.demodulate_bins ? (size_t)rd.width * rd.height * 4 : 0);
                std::vector<float> bin_albedo(o.demodulate_bins ? spectral.size() : 0);
                pt_guide_chain_desc cd;
                memset(&cd, 0, sizeof(cd));
                cd.max_chain = o.max_chain; cd.alpha_max = o.alpha_max;
                const pt_status gst = o.demodulate_bins ? pt_render_guides_bin_albedo(scene, &rd, o.guide_samples, o.chain ? &cd : nullptr, o.denoise_bins, guides.data(),
                                                                                      albedo.data(), bin_albedo.data())
                                      : o.chain ? pt_render_guides_chain(scene, &rd, o.guide_samples, &cd, guides.data(), o.demodulate ? albedo.data() : nullptr)
                                      : o.demodulate ? pt_render_guides_albedo(scene, &rd, o.guide_samples, guides.data(), albedo.data())
                                                     : pt_render_guides(scene, &rd, o.guide_samples, guides.data());
                std::vector<float> clean_spectral(spectral.size());
                const pt_status dst = gst != PT_OK ? gst
                                      : o.demodulate_bins ? pt_denoise_spectral_albedo(&dd, o.denoise_bins, film.data(), counts.data(), stats.data(), guides.data(), albedo.data(),
                                                                                       spectral.data(), bin_albedo.data(), clean.data(), clean_spectral.data(), nullptr)
                                      : o.denoise_bins ? pt_denoise_spectral(&dd, o.denoise_bins, film.data(), counts.data(), stats.data(), guides.data(), spectral.data(), clean.data(),
                                                                             clean_spectral.data(), nullptr)
                                                       : pt_denoise_film_albedo(&dd, film.data(), counts.data(), stats.data(), guides.data(), o.demodulate ? albedo.data() : nullptr,
                                                                                clean.data(), nullptr);
                if (dst != PT_OK) { fprintf(stderr, "--denoise: %s\n", pt_last_error()); rc = 1; break; }
                if (pt_output_film(&od, clean.data(), rgba.data(), linear.data()) != PT_OK) { fprintf(stderr, "pt_output_film: %s\n", pt_last_error()); rc = 1; break; }
                const std::string dbase = base + "_denoised";
                if (pt_write_exr((dbase + ".exr").c_str(), rd.width, rd.height, linear.data(), od.colorspace) != PT_OK ||
                    pt_write_png((dbase + ".png").c_str(), rd.width, rd.height, rgba.data(), od.colorspace) != PT_OK) {
                    fprintf(stderr, "failed to write files: %s\n", pt_last_error()); rc = 1; break;
                }
                if (o.write_film && !write_npy(dbase + ".npy", clean.data(), rd.height, rd.width)) { fprintf(stderr, "failed to write %s.npy\n", dbase.c_str()); rc = 1; break; }
                printf("wrote %s.exr and %s.png\n", dbase.c_str(), dbase.c_str());
                if (o.develop && o.denoise_bins && !develop(dbase + "_developed", clean_spectral.data())) { rc = 1; break; }   // (before the factor goes into the bins)
                if (o.denoise_bins && !write_spectral(dbase + "_spectral", clean_spectral)) { rc = 1; break; }   // (`linear` now holds the denoised film's R, G, B)
            }
        }
        if (scene) pt_scene_destroy(scene);
        if (rc == 0) printf("render done\n");
    }
    pt_scene_file_free(scene_file);
    pt_config_free(config);
    return rc;
}
