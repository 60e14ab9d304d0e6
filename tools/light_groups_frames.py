#!/usr/bin/env python3
"""The frames of the light-group measurement: the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2, `--spp` samples, the scene's own
1024) through pt_render and through pt_render_light_groups at G = 1, 3 and 8 (the lamp in group 0, the environment in the last), the renders alternating
`--steps` times from one process after a warm-up, each timed with the wall clock around the call (every call ends in a synchronise).  Then the mix at each G:
the resident entry against the host-array entry, `--mix-steps` times each.  `--parent-lib FILE` also times pt_render of another build of the engine (the parent
commit's libptamd.so) in the same alternation, so that the two builds' pt_render and the run-to-run spread come from one call.

Prints one JSON line: per part the median and the (min, max) of the repeats, the films compared bit for bit, the mix's yardstick bytes (G + 1) * 16 * W * H.
`--out FILE` writes the line's object to FILE.

Run it with `--kernels` under `rocprofv3 --kernel-trace --stats -- python3 tools/light_groups_frames.py --kernels` for the per-kernel times of
profiles/light_groups_kernel_stats.csv: a run of its own, pass overlap off (PT_TUNE_NO_PASS_OVERLAP), one pt_render, one group render per G and `--mix-steps`
resident mixes per G, so that the forms pt_render took, the two group forms, k_accumulate_groups and k_light_groups_mix sit in one trace of one build.
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
GROUPS = (1, 3, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions of each render")
    ap.add_argument("--mix-steps", type=int, default=10)
    ap.add_argument("--parent-lib", help="another build's libptamd.so: its pt_render is timed in the same alternation")
    ap.add_argument("--kernels", action="store_true", help="one render of each kind and the mixes, without pass overlap, for a kernel trace")
    ap.add_argument("--out", help="write the result to this file")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    a = pkg.api
    builder = pkg.scene.cornell_box()
    n_inst = len(builder.instances)
    tuning = None
    if args.kernels:
        tuning = lib.tuning_default()
        tuning.flags |= a.TUNE_NO_PASS_OVERLAP
    sc = lib.create_scene(builder, tuning=tuning)
    rd = a.render_desc(args.size, args.size, args.spp, 8, seed=1)
    warm = a.render_desc(64, 64, 10, 8, seed=1)

    def group_render(G, read_groups=True, desc=rd):
        return sc.render_light_groups(desc, [0] * n_inst, G - 1, groups=G, read_groups=read_groups)

    sc.render(warm)
    for G in GROUPS:
        group_render(G, desc=warm)   # warm-up: code objects
    if args.kernels:
        sc.render(rd)
        for G in GROUPS:
            group_render(G, read_groups=False)
            gains = a.light_group_gains(np.linspace(0.5, 1.5, G))
            for _ in range(args.mix_steps):
                sc.light_groups_mix_resident(gains)
        print(json.dumps({"mode": "kernels", "size": args.size, "spp": args.spp, "groups": GROUPS, "mix_calls_per_G": args.mix_steps, "device": lib.device_info()}))
        return

    parent = a.Library(args.parent_lib).create_scene(pkg.scene.cornell_box()) if args.parent_lib else None
    if parent:
        parent.render(warm)
    parts = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        parts.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    sc.render(rd)   # warm-up at the timed size: the queues of the frame
    same = {}
    for _ in range(args.steps):
        film, _ = timed("pt_render", lambda: sc.render(rd))
        if parent:
            pfilm, _ = timed("pt_render_parent_build", lambda: parent.render(rd))
            same["pt_render_vs_parent_build"] = bool(np.array_equal(film.view(np.uint32), pfilm.view(np.uint32)))
        for G in GROUPS:
            gfilm, groups, _ = timed("group_render_G%d" % G, lambda: group_render(G))
            same["film_G%d" % G] = bool(np.array_equal(film.view(np.uint32), gfilm.view(np.uint32)))
    mix = {}
    n = args.size * args.size
    for G in GROUPS:
        _, groups, _ = group_render(G)
        gains = a.light_group_gains(np.linspace(0.5, 1.5, G))
        res = sc.light_groups_mix_resident(gains)   # warm-up: the first call allocates the scene's mix buffer
        host = lib.light_groups_mix(groups, gains)
        for _ in range(args.mix_steps):
            res = timed("mix_resident_G%d" % G, lambda: sc.light_groups_mix_resident(gains))
            host = timed("mix_host_array_G%d" % G, lambda: lib.light_groups_mix(groups, gains))
        mix["G%d" % G] = {"yardstick_bytes": (G + 1) * 16 * n, "equal": bool(np.array_equal(res.view(np.uint32), host.view(np.uint32)))}
    summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
    result = {"size": args.size, "spp": args.spp, "steps": args.steps, "mix_steps": args.mix_steps, "seconds": summary, "bit_for_bit": same, "mix": mix,
              "parent_lib": bool(parent), "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
