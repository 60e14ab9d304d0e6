#!/usr/bin/env python3
"""Adaptive sampling (include/pt_adaptive.h) on one GPU: quality at equal time and the cost of the rounds.

  python3 tools/adaptive_quality.py [--size 512] [--spp 256] [--out profiles/adaptive_quality.json]

Quality: C2 (Cornell box, max_bounces 8, L = 2) and C3 (the gem scene, max_bounces 12, L = 2) at size x size.  Against a reference render at 16x the
fixed spp (another seed), two errors of the Y channel — RMSE / mean reference Y, and the mean per-pixel relative squared error — of
  - pt_render at the fixed spp N,
  - pt_render_adaptive (floor 20, step 20, ceiling 16 N rounded up to a multiple of 10) with the rel_error that lands at about the same wall seconds of the call (a bisection on log rel_error).
Overhead: rel_error = 0 (every pixel to max_samples, ten rounds) against pt_render at max_samples on C2 1024x1024, and the time of each round of the
equal-time C2 run (the difference of runs whose ceiling stops after k rounds), with its pixel count: what the last rounds leave of the GPU.
"""
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


def rel_rmse(film, ref):
    y, r = film[..., 1].astype(np.float64), ref[..., 1].astype(np.float64)
    return float(np.sqrt(np.mean((y - r) ** 2)) / np.mean(r))


def rel_mse(film, ref):
    """mean over pixels of (Y - Y_ref)^2 / (Y_ref^2 + (0.01 mean Y_ref)^2): every pixel's own relative error, not the lamp's edges'"""
    y, r = film[..., 1].astype(np.float64), ref[..., 1].astype(np.float64)
    return float(np.mean((y - r) ** 2 / (r * r + (0.01 * np.mean(r)) ** 2)))


def timed(fn, reps):
    """(last result, median wall seconds of the call: pt_render's and pt_render_adaptive's alike, read-backs included)"""
    out, secs = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t)
    return out, statistics.median(secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    engine = pkg.load()
    api = pkg.api
    S, N = args.size, args.spp
    record = {"command": "python3 tools/adaptive_quality.py " + " ".join(sys.argv[1:]), "device": engine.device_info(), "size": S, "fixed_spp": N,
              "reference_spp": 16 * N, "scenes": {}}
    scenes = {"C2": (pkg.scene.cornell_box, 8), "C3": (pkg.scene.cornell_gem, 12)}
    floor, step, ceiling = 20, 20, (16 * N + 9) // 10 * 10   # (pt_render_adaptive takes multiples of 10)
    for name, (make, bounces) in scenes.items():
        sc = engine.create_scene(make())
        rd = lambda spp, seed=1: api.render_desc(S, S, spp, bounces, light_samples=2, seed=seed)
        sc.render(rd(10))   # (warm-up: buffers, code objects)
        ref, _ = sc.render(rd(16 * N, seed=999))
        (fixed, fprof), t_fixed = timed(lambda: sc.render(rd(N)), args.reps)
        # bisection on log10(rel_error) for the adaptive run whose wall seconds match the fixed run's
        lo, hi, best = -4.0, 1.0, None
        for _ in range(10):
            mid = 0.5 * (lo + hi)
            (film, counts, prof), t = timed(lambda: sc.render_adaptive(rd(floor), ceiling, 10.0 ** mid, step=step), args.reps)
            cand = {"rel_error": 10.0 ** mid, "seconds": t, "mean_spp": float(counts.mean()), "min_spp": int(counts.min()), "max_spp": int(counts.max()),
                    "rounds": int(prof.kernel_launches[5]), "rel_rmse": rel_rmse(film, ref), "rel_mse": rel_mse(film, ref)}
            if best is None or abs(t - t_fixed) < abs(best["seconds"] - t_fixed):
                best = cand
            if t > t_fixed:
                lo = mid     # too slow: a looser target
            else:
                hi = mid
        entry = {"fixed": {"spp": N, "seconds": t_fixed, "rel_rmse": rel_rmse(fixed, ref), "rel_mse": rel_mse(fixed, ref)}, "adaptive_equal_time": best,
                 "adaptive_settings": {"spp": floor, "step": step, "max_samples": ceiling}}
        if name == "C2":   # the time of each round of the equal-time run
            rounds, prev = [], 0.0
            for k in range(1, best["rounds"] + 1):
                mx = min(floor + (k - 1) * step, ceiling)
                (_, counts, prof), t = timed(lambda: sc.render_adaptive(rd(floor), mx, best["rel_error"], step=step), args.reps)
                pixels = int((counts >= mx).sum())
                n_samples = floor if k == 1 else step
                rounds.append({"round": k, "pixels": pixels, "seconds": t - prev, "msamples_per_s": pixels * n_samples / max(t - prev, 1e-9) * 1e-6})
                prev = t
            entry["rounds"] = rounds
        record["scenes"][name] = entry
        print(name, json.dumps(entry, indent=1), flush=True)
    # overhead of the rounds: C2 1024x1024, rel_error 0 (20 + 9 x 20 = 200 samples in ten rounds) against pt_render at 200
    sc = engine.create_scene(pkg.scene.cornell_box())
    rd = api.render_desc(1024, 1024, 20, 8, light_samples=2, seed=1)
    sc.render(rd)
    _, t_fixed = timed(lambda: sc.render(api.render_desc(1024, 1024, 200, 8, light_samples=2, seed=1)), args.reps)
    (_, counts, prof), t_ad = timed(lambda: sc.render_adaptive(rd, 200, 0.0, step=20), args.reps)
    assert np.all(counts == 200)
    record["overhead_C2_1024"] = {"pt_render_200spp_seconds": t_fixed, "adaptive_rel0_seconds": t_ad, "rounds": int(prof.kernel_launches[5]),
                                  "overhead": t_ad / t_fixed - 1.0}
    print("overhead", json.dumps(record["overhead_C2_1024"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
