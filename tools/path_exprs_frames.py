#!/usr/bin/env python3
"""The frames of the path-expression measurement ("Path expressions"): the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2) and
scene.light_groups_room (max_bounces 5, L = 2) at `--spp` samples (120), each through pt_render_path_exprs with the eight built-in expressions
(api.PATH_PASS_EXPRS: the films of the path passes) and through its two yardsticks — pt_render_path_passes, the same films from the fixed classes, and
pt_render_light_groups at G = 8, the same planes, memsets, accumulate kernel and resident films under the group forms — the three alternating `--steps` times
from one process after a warm-up, each timed with the wall clock around the call (every call ends in a synchronise); the films are left on the device (read_*
False), so that the bus is in no number.

Prints one JSON line: per scene and entry the median and the (min, max) of the repeats, the ratios of the medians (exprs / passes, exprs / groups), each
yardstick's own run-to-run spread (max - min) / median — the margin its ratio is read against — and whether the three films are the same bits.  `--out FILE`
writes the line's object to FILE.

Run it with `--kernels --scene NAME` under `rocprofv3 --kernel-trace --stats -- python3 tools/path_exprs_frames.py --kernels --scene NAME` for the per-kernel
times of profiles/path_exprs_kernel_stats.csv: a run of its own per scene, pass overlap off (PT_TUNE_NO_PASS_OVERLAP), one render of each kind (and their
64 x 64 warm-ups, whose launches are the short ones of the minimum column), so that the three routers' forms sit in one trace of one build.
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
G = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=120)
    ap.add_argument("--steps", type=int, default=5, help="timed repetitions of each render")
    ap.add_argument("--scene", choices=("cornell_box", "light_groups_room"), help="this scene alone (a kernel trace per scene)")
    ap.add_argument("--kernels", action="store_true", help="one render of each kind per scene, without pass overlap, for a kernel trace")
    ap.add_argument("--out", help="write the result to this file")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    a = pkg.api
    tuning = None
    if args.kernels:
        tuning = lib.tuning_default()
        tuning.flags |= a.TUNE_NO_PASS_OVERLAP
    program = lib.path_expr_compile(a.PATH_PASS_EXPRS)
    scenes = {"cornell_box": (pkg.scene.cornell_box(), 8), "light_groups_room": (pkg.scene.light_groups_room(), 5)}
    result = {"size": args.size, "spp": args.spp, "steps": args.steps, "expressions": list(a.PATH_PASS_EXPRS), "states": program.states, "device": lib.device_info(),
              "scenes": {}}
    if args.scene:
        scenes = {args.scene: scenes[args.scene]}
    for name, (builder, bounces) in scenes.items():
        n_inst = len(builder.instances)
        sc = lib.create_scene(builder, tuning=tuning)
        rd = a.render_desc(args.size, args.size, args.spp, bounces, light_samples=2, seed=1)
        warm = a.render_desc(64, 64, 10, bounces, light_samples=2, seed=1)
        ids = [i % G for i in range(n_inst)]   # (every instance in some group, the environment in the last: all eight planes are live)

        def groups(desc=rd):
            return sc.render_light_groups(desc, ids, G - 1, groups=G, read_groups=False)

        def passes(desc=rd):
            return sc.render_path_passes(desc, read_passes=False)

        def exprs(desc=rd):   # (the group table given as the group render gives it, so that a lit ray looks its group up as there)
            return sc.render_path_exprs(desc, program, ids, read_films=False)

        calls = {"light_groups_G8": groups, "path_passes": passes, "path_exprs": exprs}
        for call in calls.values():   # warm-up: code objects
            call(warm)
        if args.kernels:
            for call in calls.values():
                call()
            continue
        for call in calls.values():   # warm-up at the timed size: the queues of the frame
            call()
        parts = {k: [] for k in calls}
        same = True
        for _ in range(args.steps):
            films = []
            for k, call in calls.items():
                t0 = time.perf_counter(); films.append(call()[0]); parts[k].append(time.perf_counter() - t0)
            same = same and all(bool(np.array_equal(films[0].view(np.uint32), f.view(np.uint32))) for f in films[1:])
        summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
        spread = {k: (summary[k]["max"] - summary[k]["min"]) / summary[k]["median"] for k in ("light_groups_G8", "path_passes")}
        result["scenes"][name] = {"max_bounces": bounces, "seconds": summary,
                                  "ratio_exprs_over_passes": summary["path_exprs"]["median"] / summary["path_passes"]["median"],
                                  "ratio_exprs_over_groups": summary["path_exprs"]["median"] / summary["light_groups_G8"]["median"],
                                  "yardstick_spread": spread, "film_bit_for_bit": same}
    if args.kernels:
        result = {"mode": "kernels", "size": args.size, "spp": args.spp, "scenes": list(scenes), "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
