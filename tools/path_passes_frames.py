#!/usr/bin/env python3
"""The frames of the path-pass measurement: the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2) and scene.light_groups_room
(max_bounces 5, L = 2) at `--spp` samples (120), each through pt_render_light_groups at G = 8 — the yardstick: the same planes, memsets, accumulate kernel and
resident films, with the group forms in the place of the pass forms — and through pt_render_path_passes, the two alternating `--steps` times from one process
after a warm-up, each timed with the wall clock around the call (every call ends in a synchronise); the films are left on the device (read_groups / read_passes
False), so that the bus is in neither number.

Prints one JSON line: per scene and entry the median and the (min, max) of the repeats, the ratio of the medians (passes / groups), the yardstick's own
run-to-run spread (max - min) / median — the margin the ratio is read against — and whether the two films are the same bits.  `--out FILE` writes the line's
object to FILE.

Run it with `--kernels --scene NAME` under `rocprofv3 --kernel-trace --stats -- python3 tools/path_passes_frames.py --kernels --scene NAME` for the per-kernel
times of profiles/path_passes_kernel_stats.csv: a run of its own per scene, pass overlap off (PT_TUNE_NO_PASS_OVERLAP), one render of each kind (and their
64 x 64 warm-ups, whose launches are the short ones of the minimum column), so that the two group forms and the two pass forms sit in one trace of one build.
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
    scenes = {"cornell_box": (pkg.scene.cornell_box(), 8), "light_groups_room": (pkg.scene.light_groups_room(), 5)}
    result = {"size": args.size, "spp": args.spp, "steps": args.steps, "groups": G, "device": lib.device_info(), "scenes": {}}
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

        groups(warm); passes(warm)   # warm-up: code objects
        if args.kernels:
            groups(); passes()
            continue
        groups(); passes()           # warm-up at the timed size: the queues of the frame
        parts = {"light_groups_G8": [], "path_passes": []}
        same = True
        for _ in range(args.steps):
            t0 = time.perf_counter(); gfilm = groups()[0]; parts["light_groups_G8"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); pfilm = passes()[0]; parts["path_passes"].append(time.perf_counter() - t0)
            same = same and bool(np.array_equal(gfilm.view(np.uint32), pfilm.view(np.uint32)))
        summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
        y = summary["light_groups_G8"]
        result["scenes"][name] = {"max_bounces": bounces, "seconds": summary, "ratio_passes_over_groups": summary["path_passes"]["median"] / y["median"],
                                  "yardstick_spread": (y["max"] - y["min"]) / y["median"], "film_bit_for_bit": same}
    if args.kernels:
        result = {"mode": "kernels", "size": args.size, "spp": args.spp, "groups": G, "scenes": list(scenes), "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
