#!/usr/bin/env python3
"""The frame of the joint filter's measurement ("Denoising the bins"): the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2)
through pt_render_adaptive_spectral at `--bins` bins (spp `--spp`, up to `--max-samples` in rounds of `--step`, relative error `--rel-error`), its guides,
pt_denoise_spectral, and — for the yardstick, from the same film — pt_denoise_film, after one warm-up of each.  Prints one JSON line with the wall
seconds of the calls (host arrays in and out: transfers and allocations included) and the bytes a pass of the gather moves.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/denoise_spectral_frames.py` for the per-kernel times of profiles/denoise_spectral_kernel_stats.csv:
k_dn_gather_spectral next to k_dn_gather, k_adaptive_finish_spectral, and k_accumulate_spectral under adaptive rounds, all of one build.
With `--bin-albedo` the frame also goes through pt_render_guides_bin_albedo (next to pt_render_guides_albedo, the yardstick of its fold) and
pt_denoise_spectral_albedo: the run behind profiles/denoise_spectral_albedo_kernel_stats.csv (k_guide_fold_bins, k_dn_demodulate_bins, k_dn_remodulate_bins).
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=40)
    ap.add_argument("--max-samples", type=int, default=120)
    ap.add_argument("--step", type=int, default=40)
    ap.add_argument("--rel-error", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions of the two filter calls")
    ap.add_argument("--bin-albedo", action="store_true", help="also the per-bin albedo guide and the filter that demodulates the bins by it")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    sc = lib.create_scene(pkg.scene.cornell_box())
    rd = pkg.api.render_desc(args.size, args.size, args.spp, 8, seed=1)
    sc.render_adaptive_spectral(pkg.api.render_desc(64, 64, args.spp, 8, seed=1), args.bins, args.spp, 0.0)   # warm-up: code objects
    t = time.perf_counter()
    film, counts, st, spectral, prof = sc.render_adaptive_spectral(rd, args.bins, args.max_samples, args.rel_error, step=args.step, stats=True)
    t_render = time.perf_counter() - t
    guides = sc.render_guides(rd, 4)

    def timed(fn):
        fn()
        secs = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            secs.append(time.perf_counter() - t0)
        return sorted(secs)[len(secs) // 2]
    t_joint = timed(lambda: lib.denoise_spectral(film, counts, st, guides, spectral))
    t_film = timed(lambda: lib.denoise_film(film, counts, st, guides))
    extra = {}
    if args.bin_albedo:
        t_guides_albedo = timed(lambda: sc.render_guides_albedo(rd, 4))
        t_guides_bins = timed(lambda: sc.render_guides_bin_albedo(rd, args.bins, 4))
        _, albedo, bin_albedo = sc.render_guides_bin_albedo(rd, args.bins, 4)
        t_demod = timed(lambda: lib.denoise_spectral_albedo(film, counts, st, guides, spectral, albedo, bin_albedo))
        extra = {"guides_albedo_seconds": t_guides_albedo, "guides_bin_albedo_seconds": t_guides_bins, "denoise_spectral_albedo_seconds": t_demod,
                 "demodulate_bytes": 3 * args.bins * 4 * args.size * args.size}
    n = args.size * args.size
    print(json.dumps({"bins": args.bins, "size": args.size, "spp": args.spp, "max_samples": args.max_samples, "step": args.step, "rel_error": args.rel_error,
                      "rounds": int(prof.kernel_launches[5]), "mean_samples": float(counts.mean()), "render_seconds": t_render,
                      "denoise_spectral_seconds": t_joint, "denoise_film_seconds": t_film,
                      "plane_bytes_per_pass": 2 * args.bins * 4 * n, "device": lib.device_info(), **extra}))


if __name__ == "__main__":
    main()
