#!/usr/bin/env python3
"""The frame of the assemble's measurement ("Assembling a node render"): the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2) through
pt_render_adaptive_spectral_multi on `--virtual` virtual devices of device 0 at `--bins` bins (spp `--spp`, up to `--max-samples` in rounds of `--step`,
relative error `--rel-error`), then three routes from the node render to the denoised set, nothing read back:

  (a) load       resident_load of the arrays the render returned, resident_guides(albedo, bin_albedo), denoise_resident
  (b) assemble   resident_assemble, the same guides, the same filter
  (c) staged     (b) with resident_assemble(staged=True): every shard through the staging copy, the route a shard on another device takes

All three are warmed — that pass reads the denoised film, its variance and the denoised bins back, and the three routes' must be equal bit for bit, else the
program ends with status 1 —, then run alternately `--steps` times from one process; every part is timed on its own with the wall clock (each call ends in a
synchronise).  Prints one JSON line: per part the median and the (min, max) of the repeats, and the routes' totals.  `--out FILE` appends the line's object
to a JSON list in FILE.

Run it with `--kernels` under `rocprofv3 --kernel-trace --stats -- python3 tools/resident_assemble_frames.py --kernels` for the per-kernel times of
profiles/resident_assemble_kernel_stats.csv: that mode renders and assembles `--steps` times, in place and staged, so that k_spectral_pack's dispatches (one per
shard and render) and k_spectral_unpack's (one per shard and assemble) over the same shards sit in one trace of one build.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

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
    ap.add_argument("--virtual", type=int, default=4, help="virtual devices on device 0 (pt_tuning::multi_virtual)")
    ap.add_argument("--steps", type=int, default=7, help="timed repetitions of each route")
    ap.add_argument("--kernels", action="store_true", help="renders and assembles alone, for a kernel trace")
    ap.add_argument("--out", help="append the result to the JSON list in this file")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    tuning = lib.tuning_default()
    tuning.multi_virtual = args.virtual
    sc = lib.create_scene(pkg.scene.cornell_box(), tuning)
    rd = pkg.api.render_desc(args.size, args.size, args.spp, 8, seed=1)

    def render():
        return sc.render_adaptive_spectral_multi(rd, args.bins, args.max_samples, args.rel_error, step=args.step, stats=True, device_mask=1)
    sc.render_adaptive_spectral_multi(pkg.api.render_desc(64, 64, args.spp, 8, seed=1), args.bins, args.spp, 0.0, stats=True, device_mask=1)   # warm-up: code objects, replicas

    if args.kernels:
        for _ in range(args.steps):
            render()
            sc.resident_assemble()
            sc.resident_assemble(staged=True)
        print(json.dumps({"mode": "kernels", "bins": args.bins, "size": args.size, "virtual": args.virtual, "renders": args.steps, "assembles": 2 * args.steps,
                          "device": lib.device_info()}))
        return

    t = time.perf_counter()
    film, counts, st, spectral, prof = render()
    t_render = time.perf_counter() - t
    parts = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        parts.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def route(name, first):
        timed(name, first)
        timed(name + "_guides", lambda: sc.resident_guides(rd, 4, albedo=True, bin_albedo=True))
        timed(name + "_filter", lambda: sc.denoise_resident(film=False))

    routes = (("load", lambda: sc.resident_load(film, counts, st, spectral=spectral)),
              ("assemble", lambda: sc.resident_assemble()),
              ("staged", lambda: sc.resident_assemble(staged=True)))
    outputs = {}
    for name, first in routes:   # warm all three (code objects, the scene's kept buffers), and keep what each returns
        route(name, first)
        outputs[name] = sc.denoise_resident(variance=True, spectral=True)
    same = {name: all(bool(np.array_equal(x.view(np.uint32), y.view(np.uint32))) for x, y in zip(outputs[name], outputs["load"])) for name in ("assemble", "staged")}
    parts.clear()
    for _ in range(args.steps):
        for name, first in routes:
            route(name, first)
    summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
    total = lambda name: sum(summary[n]["median"] for n in (name, name + "_guides", name + "_filter"))
    n = args.size * args.size
    result = {"bins": args.bins, "size": args.size, "spp": args.spp, "max_samples": args.max_samples, "step": args.step, "rel_error": args.rel_error,
              "virtual": args.virtual, "physical_devices": 1, "steps": args.steps, "rounds": int(prof.kernel_launches[5]), "mean_samples": float(counts.mean()),
              "render_seconds": t_render, "render_exchange_seconds": float(prof.kernel_seconds[6]), "seconds": summary,
              "route_seconds": {name: total(name) for name, _ in routes}, "bit_for_bit_with_load": same,
              "film_counts_stats_bytes": 36 * n, "bin_bytes": args.bins * 4 * n, "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else []
        json.dump(old + [result], open(args.out, "w"), indent=1)
    if not all(same.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
