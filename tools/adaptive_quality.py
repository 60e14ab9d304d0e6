#!/usr/bin/env python3
"""Adaptive sampling (include/pt_adaptive.h) on one GPU: quality at equal time and the cost of the rounds.

  python3 tools/adaptive_quality.py [--size 512] [--spp 256] [--out profiles/adaptive_quality.json]
                                    [--scenes C2,C3] [--devices MASK] [--virtual V] [--rccl] [--no-overhead]

Quality: C2 (Cornell box, max_bounces 8, L = 2) and C3 (the gem scene, max_bounces 12, L = 2) at size x size.  Against a reference render at 16x the
fixed spp (another seed), two errors of the Y channel — RMSE / mean reference Y, and the mean per-pixel relative squared error — of
  - pt_render at the fixed spp N,
  - pt_render_adaptive (floor 20, step 20, ceiling 16 N rounded up to a multiple of 10) with the rel_error that lands at about the same wall seconds of the call (a bisection on log rel_error).
Overhead: rel_error = 0 (every pixel to max_samples, ten rounds) against pt_render at max_samples on C2 1024x1024, and the time of each round of the
equal-time C2 run (the difference of runs whose ceiling stops after k rounds), with its pixel count: what the last rounds leave of the GPU.

--devices / --virtual run every adaptive render through pt_render_adaptive_multi on the devices of MASK, each treated as V virtual devices
(pt_tuning::multi_virtual; --rccl forces the RCCL exchange and gather, PT_TUNE_MULTI_RCCL).  The record then holds, per scene, the cost of the exchange:
profile.kernel_seconds[6] of the equal-time run (every round's exchange plus the final gather), the gather alone (a one-round run, which exchanges
nothing) and their difference per exchanging round.
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
    ap.add_argument("--scenes", default="C2,C3", help="comma-separated subset of C2,C3")
    ap.add_argument("--devices", type=lambda v: int(v, 0), default=None, help="device mask for pt_render_adaptive_multi (0 = all)")
    ap.add_argument("--virtual", type=int, default=0, help="virtual devices per device (pt_tuning::multi_virtual); implies --devices 1 if not given")
    ap.add_argument("--rccl", action="store_true", help="force the RCCL exchange and gather (PT_TUNE_MULTI_RCCL)")
    ap.add_argument("--no-overhead", action="store_true", help="skip the rel_error = 0 overhead run on C2 1024x1024")
    args = ap.parse_args()
    multi = args.devices is not None or args.virtual > 1 or args.rccl
    mask = args.devices if args.devices is not None else 1
    pkg = importlib.import_module("rust-pathtracer_amd")
    engine = pkg.load()
    api = pkg.api
    S, N = args.size, args.spp
    record = {"command": "python3 tools/adaptive_quality.py " + " ".join(sys.argv[1:]), "device": engine.device_info(), "size": S, "fixed_spp": N,
              "reference_spp": 16 * N, "scenes": {}}
    if multi:
        record["multi"] = {"device_mask": mask, "virtual": max(args.virtual, 1), "rccl": args.rccl}
    scenes = {k: v for k, v in {"C2": (pkg.scene.cornell_box, 8), "C3": (pkg.scene.cornell_gem, 12)}.items() if k in args.scenes.split(",")}

    def make_scene(builder):
        if not multi:
            return engine.create_scene(builder)
        t = engine.tuning_default()
        t.multi_virtual = args.virtual
        if args.rccl:
            t.flags |= api.TUNE_MULTI_RCCL
        return engine.create_scene(builder, t)

    def adaptive(sc, rd, mx, rel, step):
        return sc.render_adaptive_multi(rd, mx, rel, step=step, device_mask=mask) if multi else sc.render_adaptive(rd, mx, rel, step=step)
    floor, step, ceiling = 20, 20, (16 * N + 9) // 10 * 10   # (pt_render_adaptive takes multiples of 10)
    for name, (make, bounces) in scenes.items():
        sc = make_scene(make())
        rd = lambda spp, seed=1: api.render_desc(S, S, spp, bounces, light_samples=2, seed=seed)
        sc.render(rd(10))   # (warm-up: buffers, code objects)
        ref, _ = sc.render(rd(16 * N, seed=999))
        (fixed, fprof), t_fixed = timed(lambda: sc.render(rd(N)), args.reps)
        # bisection on log10(rel_error) for the adaptive run whose wall seconds match the fixed run's
        lo, hi, best = -4.0, 1.0, None
        for _ in range(10):
            mid = 0.5 * (lo + hi)
            (film, counts, prof), t = timed(lambda: adaptive(sc, rd(floor), ceiling, 10.0 ** mid, step), args.reps)
            cand = {"rel_error": 10.0 ** mid, "seconds": t, "mean_spp": float(counts.mean()), "min_spp": int(counts.min()), "max_spp": int(counts.max()),
                    "rounds": int(prof.kernel_launches[5]), "rel_rmse": rel_rmse(film, ref), "rel_mse": rel_mse(film, ref)}
            if multi:
                cand["exchange_and_gather_seconds"] = prof.kernel_seconds[6]
            if best is None or abs(t - t_fixed) < abs(best["seconds"] - t_fixed):
                best = cand
            if t > t_fixed:
                lo = mid     # too slow: a looser target
            else:
                hi = mid
        entry = {"fixed": {"spp": N, "seconds": t_fixed, "rel_rmse": rel_rmse(fixed, ref), "rel_mse": rel_mse(fixed, ref)}, "adaptive_equal_time": best,
                 "adaptive_settings": {"spp": floor, "step": step, "max_samples": ceiling}}
        if multi:   # the gather alone: one round (max_samples = the floor) exchanges nothing
            gathers = [adaptive(sc, rd(floor), floor, best["rel_error"], step)[2].kernel_seconds[6] for _ in range(args.reps)]
            g = statistics.median(gathers)
            entry["exchange"] = {"gather_seconds": g, "rounds": best["rounds"], "exchange_and_gather_seconds": best["exchange_and_gather_seconds"],
                                 "per_round_exchange_seconds": (best["exchange_and_gather_seconds"] - g) / max(best["rounds"] - 1, 1)}
        if name == "C2":   # the time of each round of the equal-time run
            rounds, prev = [], 0.0
            for k in range(1, best["rounds"] + 1):
                mx = min(floor + (k - 1) * step, ceiling)
                (_, counts, prof), t = timed(lambda: adaptive(sc, rd(floor), mx, best["rel_error"], step), args.reps)
                pixels = int((counts >= mx).sum())
                n_samples = floor if k == 1 else step
                rounds.append({"round": k, "pixels": pixels, "seconds": t - prev, "msamples_per_s": pixels * n_samples / max(t - prev, 1e-9) * 1e-6})
                prev = t
            entry["rounds"] = rounds
        record["scenes"][name] = entry
        print(name, json.dumps(entry, indent=1), flush=True)
    # overhead of the rounds: C2 1024x1024, rel_error 0 (20 + 9 x 20 = 200 samples in ten rounds) against pt_render at 200
    if args.no_overhead:
        if args.out:
            with open(args.out, "w") as f:
                json.dump(record, f, indent=1)
        return
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
