#!/usr/bin/env python3
"""The film denoiser (include/pt_denoise.h): what it buys and what it costs.

  python3 tools/denoise_quality.py [--size 256] [--spp 20,40,80] [--ref-spp 4096] [--out profiles/denoise_quality.json]
  python3 tools/denoise_quality.py --emulation [--out ...]     the definition on the CPU (48x48, 20 spp against 1000 spp: the case tests/test_denoise.py asserts)
  python3 tools/denoise_quality.py --one-pass 1024             one 1024x1024 render, guides and filter call (the program to run under rocprofv3 --kernel-trace --stats)
  python3 tools/denoise_quality.py --one-pass 1024 --demodulate   the same on cornell_checker, the guides and the filter once without and once with the albedo
  python3 tools/denoise_quality.py --library PATH --key NAME   another build of the engine (entries it lacks are left out)
  python3 tools/denoise_quality.py --chain 8 [--emulation]     specular-chain guides against first-hit guides (key gpu_<size>_chain / emulation_48_chain): the demodulated filter
                                                               on cornell_checker_slab and cornell_gem, and the wall time of the two guide passes there and on cornell_checker
  python3 tools/denoise_quality.py --one-pass 1024 --demodulate --chain 8 [--scene cornell_checker_slab]   one render, both guide passes, both filter calls
  python3 tools/denoise_quality.py --spectral-bins 8 [--size 32 --spp 20 --ref-spp 4000]   the joint filter of the film and its bins (pt_denoise_spectral, key gpu_<size>_spectral<B>):
                                                               per scene and spp also the summed squared error of the noisy and of the denoised bins against a converged pt_render_spectral
  python3 tools/denoise_quality.py --spectral-bins 8 --bin-albedo [--size 32 --spp 20 --ref-spp 4000]   the bins through pt_denoise_spectral and through
                                                               pt_denoise_spectral_albedo with pt_render_guides_bin_albedo's per-bin albedo (key gpu_<size>_spectral<B>_bin_albedo):
                                                               on cornell_checker(rgba=True), cornell_checker and cornell_box the summed squared error of the noisy, the filtered and
                                                               the demodulated-filter bins, over the whole film and over the pixels whose sample-0 ray hits the checker

Quality: Cornell box, the gem scene, mixed_primitives, hdri_small and cornell_checker at size x size, max_bounces 6, seed 1, the defaults of pt_denoise_desc,
guides of 4 samples.  Against a reference render of another seed (77), RMSE over XYZ of the noisy film, of the denoised film and of the film denoised with
albedo demodulation, their ratios, and the shift of the mean Y; for cornell_checker also over the pixels whose sample-0 camera ray hits the checker.
Cost: median wall seconds of pt_render_guides(_albedo) and pt_denoise_film(_albedo) (host arrays in and out: transfers and allocations included) beside the render's.
--out merges into an existing file: the GPU run and the emulation run fill their own keys."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = ("cornell_box", "cornell_gem", "mixed_primitives", "hdri_small", "cornell_checker")
BOUNCES = 6


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def timed(fn, reps):
    out, secs = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t)
    return out, statistics.median(secs)


def emulation_library(pkg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emulation
    return emulation.load(pkg, "guides_chain")


def checker_mask(sc, builder, rd):
    """The pixels whose sample-0 camera ray hits cornell_checker's checker."""
    n = rd.width * rd.height
    o, d, _ = sc.camera_samples(rd, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32))
    h = sc.intersect(o, d)
    return ((h["valid"] != 0) & (h["material"] == builder.material("checker"))).reshape(rd.height, rd.width)


def chain_walk(pkg, lib, sc, builder, rd, K, D):
    """The chains of samples 0 .. K-1 walked in numpy from the probes (the restatement tests/test_guides_chain.py checks the emulation against): per sample how
    it ended, what it passed, and the rays traced per chain vertex."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_guides_chain as tgc
    return tgc, tgc.np_chain(pkg.api, lib, sc, builder, rd, K, D, want_albedo=False)[2]


def measure_chain(lib, pkg, name, size, spps, ref, reps, D):
    """Chain guides (max_chain D) against first-hit guides, both with their albedo and the demodulated filter, on one noisy film per spp; the wall time of the
    two guide passes (median, minimum and maximum of `reps` calls).  specular_*: over the pixels whose sample-0 chain follows at least one vertex; on
    cornell_checker_slab checker_*: over those whose sample-0 chain crosses the slab and ends on the checker."""
    builder = getattr(pkg.scene, name)()
    sc = lib.create_scene(builder)
    rd = pkg.api.render_desc(size, size, spps[0], BOUNCES, seed=1)
    out = {"max_chain": D, "guide_seconds": {}}
    passes = {}
    for tag, fn in (("first_hit", lambda: sc.render_guides_albedo(rd, 4)), ("chain", lambda: sc.render_guides_chain(rd, 4, D))):
        fn()
        secs = []
        for _ in range(reps):
            t = time.perf_counter()
            passes[tag] = fn()
            secs.append(time.perf_counter() - t)
        out["guide_seconds"][tag] = {"median": statistics.median(secs), "min": min(secs), "max": max(secs), "runs": reps}
    tgc, diag = chain_walk(pkg, lib, sc, builder, rd, 4, D)
    out["rays_per_vertex"] = [sum(dg["rounds"][v] for dg in diag if v < len(dg["rounds"])) for v in range(D + 1)]
    out["loop_rounds_per_sample"] = [len(dg["rounds"]) for dg in diag]
    masks = {"specular": (diag[0]["vertex"] > 0).reshape(size, size)}
    if name == "cornell_checker_slab":
        crossed = np.zeros(size * size, bool)
        for p in diag[0]["passed"]:
            crossed |= p == builder.material("ggx_glass")
        masks["checker"] = (crossed & (diag[0]["end"] == tgc.END_TERMINAL) & (diag[0]["material"] == builder.material("checker"))).reshape(size, size)
    out["pixels"] = {k: int(m.sum()) for k, m in masks.items()}
    out["spp"] = []
    for spp in spps:
        rds = pkg.api.render_desc(size, size, spp, BOUNCES, seed=1)
        film, counts, st, _ = sc.render_adaptive(rds, spp, 0.0, stats=True)
        films = {"noisy": film}
        for tag, (g, a) in passes.items():
            films[tag] = lib.denoise_film(film, counts, st, g, albedo=a)
        rec = {"spp": spp}
        for tag, f in films.items():
            rec["rmse_" + tag] = rmse(f, ref)
            for k, m in masks.items():
                if m.any():
                    rec[k + "_rmse_" + tag] = rmse(f[m], ref[m])
        rec["ratio_chain_to_first_hit"] = rec["rmse_chain"] / rec["rmse_first_hit"]
        for k, m in masks.items():
            if m.any():
                rec[k + "_ratio_chain_to_first_hit"] = rec[k + "_rmse_chain"] / rec[k + "_rmse_first_hit"]
        out["spp"].append(rec)
    return out


def sse(a, b):
    return float(np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def measure(lib, pkg, name, size, spp, ref, reps, bins=0, ref_spectral=None):
    """`bins` > 0: the render is render_adaptive_spectral (the same film, counts and statistics) and the record gains the summed squared error, over every bin
    and pixel, of its bins and of denoise_spectral's against ref_spectral."""
    builder = getattr(pkg.scene, name)()
    sc = lib.create_scene(builder)
    rd = pkg.api.render_desc(size, size, spp, BOUNCES, seed=1)
    spectral = None
    if bins:
        (film, counts, st, spectral, _), t_render = timed(lambda: sc.render_adaptive_spectral(rd, bins, spp, 0.0, stats=True), reps)
    else:
        (film, counts, st, _), t_render = timed(lambda: sc.render_adaptive(rd, spp, 0.0, stats=True), reps)
    guides, t_guides = timed(lambda: sc.render_guides(rd, 4), reps)
    den, t_filter = timed(lambda: lib.denoise_film(film, counts, st, guides), reps)
    e0, e1 = rmse(film, ref), rmse(den, ref)
    out = {"spp": spp, "rmse_noisy": e0, "rmse_denoised": e1, "ratio": e1 / e0, "mean_y_noisy": float(film[..., 1].mean()), "mean_y_denoised": float(den[..., 1].mean()),
           "mean_y_shift": float(den[..., 1].mean() / film[..., 1].mean() - 1.0), "render_seconds": t_render, "guides_seconds": t_guides, "filter_seconds": t_filter}
    films = {"noisy": film, "denoised": den}
    if bins:
        (_, den_spectral), out["filter_spectral_seconds"] = timed(lambda: lib.denoise_spectral(film, counts, st, guides, spectral), reps)
        e0, e1 = sse(spectral, ref_spectral), sse(den_spectral, ref_spectral)
        out.update({"bins": bins, "sse_bins_noisy": e0, "sse_bins_denoised": e1, "sse_bins_ratio": e1 / e0})
    if lib._render_guides_albedo is not None:
        (_, albedo), out["guides_albedo_seconds"] = timed(lambda: sc.render_guides_albedo(rd, 4), reps)
        dem, out["filter_albedo_seconds"] = timed(lambda: lib.denoise_film(film, counts, st, guides, albedo=albedo), reps)
        e2 = rmse(dem, ref)
        out.update({"rmse_demodulated": e2, "ratio_demodulated": e2 / e0, "mean_y_shift_demodulated": float(dem[..., 1].mean() / film[..., 1].mean() - 1.0)})
        films["demodulated"] = dem
    if name == "cornell_checker":
        mask = checker_mask(sc, builder, rd)
        out["checker_pixels"] = int(mask.sum())
        for k, f in films.items():
            out["checker_rmse_" + k] = rmse(f[mask], ref[mask])
    return out


def measure_bin_albedo(lib, pkg, name, size, spp, ref_spp, reps, bins):
    """The bins of one noisy render_adaptive_spectral through denoise_spectral and through denoise_spectral_albedo (guides, XYZ albedo and per-bin albedo of 4
    samples from one render_guides_bin_albedo call), against render_spectral at ref_spp of seed 77."""
    builder = pkg.scene.cornell_checker(rgba=True) if name == "cornell_checker_rgba" else getattr(pkg.scene, name)()
    sc = lib.create_scene(builder)
    rd = pkg.api.render_desc(size, size, spp, BOUNCES, seed=1)
    _, ref, _ = sc.render_spectral(pkg.api.render_desc(size, size, ref_spp, BOUNCES, seed=77), bins)
    film, counts, st, spectral, _ = sc.render_adaptive_spectral(rd, bins, spp, 0.0, stats=True)
    (guides, albedo, bin_albedo), t_guides = timed(lambda: sc.render_guides_bin_albedo(rd, bins, 4), reps)
    _, t_guides_albedo = timed(lambda: sc.render_guides_albedo(rd, 4), reps)
    (_, plain), t_plain = timed(lambda: lib.denoise_spectral(film, counts, st, guides, spectral), reps)
    (_, demod), t_demod = timed(lambda: lib.denoise_spectral_albedo(film, counts, st, guides, spectral, albedo, bin_albedo), reps)
    out = {"spp": spp, "bins": bins, "sse_bins_noisy": sse(spectral, ref), "sse_bins_denoised": sse(plain, ref), "sse_bins_demodulated": sse(demod, ref),
           "guides_bin_albedo_seconds": t_guides, "guides_albedo_seconds": t_guides_albedo, "filter_spectral_seconds": t_plain, "filter_spectral_albedo_seconds": t_demod}
    out["sse_bins_demodulated_to_denoised"] = out["sse_bins_demodulated"] / out["sse_bins_denoised"]
    if name.startswith("cornell_checker"):
        mask = checker_mask(sc, builder, rd)
        out["checker_pixels"] = int(mask.sum())
        for k, f in (("noisy", spectral), ("denoised", plain), ("demodulated", demod)):
            out["checker_sse_bins_" + k] = sse(f[:, mask], ref[:, mask])
        out["checker_sse_bins_demodulated_to_denoised"] = out["checker_sse_bins_demodulated"] / out["checker_sse_bins_denoised"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", default=None, help="default 20,40,80; with --emulation 20")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--emulation", action="store_true")
    ap.add_argument("--one-pass", type=int, default=0, metavar="SIZE")
    ap.add_argument("--demodulate", action="store_true", help="--one-pass: cornell_checker, without and with the albedo")
    ap.add_argument("--chain", type=int, default=None, metavar="D", help="specular-chain guides of max_chain D against first-hit guides")
    ap.add_argument("--scene", default="cornell_checker_slab", help="--one-pass --chain: the scene")
    ap.add_argument("--rounds", action="store_true", help="--one-pass --chain: also print the rays traced per chain vertex (a numpy walk over the probes)")
    ap.add_argument("--spectral-bins", type=int, default=0, metavar="B", help="also the bins' summed squared errors through the joint filter (not with --emulation: it renders no spectral film)")
    ap.add_argument("--bin-albedo", action="store_true", help="--spectral-bins: the bins with and without demodulation by the per-bin albedo (its own key and scenes)")
    ap.add_argument("--library", default=None, metavar="PATH", help="another build of libptamd.so")
    ap.add_argument("--key", default=None, help="the record's key in --out (default gpu_<size> / emulation_48)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    if args.spectral_bins and (args.one_pass or args.emulation or args.chain is not None):
        ap.error("--spectral-bins measures the engine's joint filter in the quality record: not with --one-pass, --emulation or --chain")
    if args.bin_albedo and not args.spectral_bins:
        ap.error("--bin-albedo needs --spectral-bins")
    if args.one_pass:
        engine = pkg.load()
        rd = pkg.api.render_desc(args.one_pass, args.one_pass, 20, BOUNCES, seed=1)
        if args.chain is not None:
            builder = getattr(pkg.scene, args.scene)()
            sc = engine.create_scene(builder)
            film, counts, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
            g0, a0 = sc.render_guides_albedo(rd, 4)
            g1, a1 = sc.render_guides_chain(rd, 4, args.chain)
            first, chain = engine.denoise_film(film, counts, st, g0, albedo=a0), engine.denoise_film(film, counts, st, g1, albedo=a1)
            print("%s %dx%d, max_chain %d: mean Y %.6g -> first-hit guides %.6g, chain guides %.6g"
                  % (args.scene, args.one_pass, args.one_pass, args.chain, film[..., 1].mean(), first[..., 1].mean(), chain[..., 1].mean()))
            if args.rounds:   # (not under a profiler: the walk traces its rays through the probe too)
                _, diag = chain_walk(pkg, engine, sc, builder, rd, 4, args.chain)
                print("rays per chain vertex, samples 0..3: %s" % [dg["rounds"] for dg in diag])
            return
        if args.demodulate:
            sc = engine.create_scene(pkg.scene.cornell_checker())
            film, counts, st, _ = sc.render_adaptive(rd, 20, 0.0, stats=True)
            guides = sc.render_guides(rd, 4)
            _, albedo = sc.render_guides_albedo(rd, 4)
            den, dem = engine.denoise_film(film, counts, st, guides), engine.denoise_film(film, counts, st, guides, albedo=albedo)
            print("denoised %dx%d: mean Y %.6g -> %.6g, demodulated %.6g" % (args.one_pass, args.one_pass, film[..., 1].mean(), den[..., 1].mean(), dem[..., 1].mean()))
            return
        sc = engine.create_scene(pkg.scene.cornell_box())
        film, den, counts, _ = sc.render_denoised(rd)
        print("denoised %dx%d: mean Y %.6g -> %.6g" % (args.one_pass, args.one_pass, film[..., 1].mean(), den[..., 1].mean()))
        return
    if args.emulation:
        lib, key, size, spps, ref_spp, reps = emulation_library(pkg), "emulation_48", 48, [int(s) for s in (args.spp or "20").split(",")], 1000, 1
    else:
        lib = pkg.api.Library(args.library, "pt_") if args.library else pkg.load()
        key, size, spps, ref_spp, reps = "gpu_%d" % args.size, args.size, [int(s) for s in (args.spp or "20,40,80").split(",")], args.ref_spp, args.reps
    if args.chain is not None:
        key += "_chain"
    if args.spectral_bins:
        key += "_spectral%d" % args.spectral_bins
    if args.bin_albedo:
        key += "_bin_albedo"
    key = args.key or key
    record = {"command": "python3 tools/denoise_quality.py " + " ".join(sys.argv[1:]), "device": "host emulation (CPU)" if args.emulation else lib.device_info(), "size": size, "reference_spp": ref_spp,
              "reference_seed": 77, "max_bounces": BOUNCES, "guide_samples": 4, "scenes": {}}
    for name in (("cornell_checker_slab", "cornell_gem", "cornell_checker") if args.chain is not None else ()):
        ref, _ = lib.create_scene(getattr(pkg.scene, name)()).render(pkg.api.render_desc(size, size, ref_spp, BOUNCES, seed=77))
        record["scenes"][name] = measure_chain(lib, pkg, name, size, spps, ref, 5 if not args.emulation else 1, args.chain)
        print(name, json.dumps(record["scenes"][name], indent=1), flush=True)
    for name in (("cornell_checker_rgba", "cornell_checker", "cornell_box") if args.bin_albedo else ()):
        record["scenes"][name] = [measure_bin_albedo(lib, pkg, name, size, spp, ref_spp, reps, args.spectral_bins) for spp in spps]
        print(name, json.dumps(record["scenes"][name], indent=1), flush=True)
    for name in (SCENES if args.chain is None and not args.bin_albedo else ()):
        ref_rd, ref_spectral = pkg.api.render_desc(size, size, ref_spp, BOUNCES, seed=77), None
        if args.spectral_bins:   # (render_spectral's film is render's)
            ref, ref_spectral, _ = lib.create_scene(getattr(pkg.scene, name)()).render_spectral(ref_rd, args.spectral_bins)
        else:
            ref, _ = lib.create_scene(getattr(pkg.scene, name)()).render(ref_rd)
        record["scenes"][name] = [measure(lib, pkg, name, size, spp, ref, reps, args.spectral_bins, ref_spectral) for spp in spps]
        print(name, json.dumps(record["scenes"][name], indent=1), flush=True)
    if args.out:
        whole = json.load(open(args.out)) if os.path.exists(args.out) else {}
        whole[key] = record
        with open(args.out, "w") as f:
            json.dump(whole, f, indent=1)


if __name__ == "__main__":
    main()
