#!/usr/bin/env python3
"""The quality table of the denoised light groups on the engine: light_groups_room at `--sizes` (32 and a larger size), `--spp` samples,
5 bounces, L = 2, seed 7, every emitter a group of its own, through render_denoised_light_groups with and without albedo demodulation, against a group render
of `--reference-spp` samples with seed 99.  Per group, for the total film and for several gain sets: the squared error of the XYZ channels of the noisy and of
the denoised films against the reference, and their ratio.  A ratio above 1 is listed under "worse": it is reported, not tuned away.

Prints one JSON line; `--out FILE` writes the line's object to FILE."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOM_GROUPS, ROOM_ENV_GROUP = (0, 0, 1, 0, 0, 0), 2   # instance 1 the rect lamp, instance 2 the disk lamp, the environment the third group
GAINS = [(1.0, 1.0, 1.0), (0.25, 4.0, 0.25), (4.0, 0.25, 0.25), (0.25, 0.25, 4.0), (0.0, 1.0, 0.0), (1.0, 0.0, 1.0)]


def sq_err(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--spp", type=int, default=20)
    ap.add_argument("--reference-spp", type=int, default=1280)
    ap.add_argument("--out", help="write the result to this file")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    a = pkg.api
    result = {"scene": "light_groups_room", "spp": args.spp, "reference_spp": args.reference_spp, "groups": ["rect lamp", "disk lamp", "environment"], "sizes": {},
              "worse": [], "device": lib.device_info()}
    for size in args.sizes:
        sc = lib.create_scene(pkg.scene.light_groups_room())
        ref_film, ref_groups, _ = sc.render_light_groups(a.render_desc(size, size, args.reference_spp, 5, light_samples=2, seed=99), ROOM_GROUPS, ROOM_ENV_GROUP)
        rd = a.render_desc(size, size, args.spp, 5, light_samples=2, seed=7)
        table = {}
        for albedo in (False, True):
            film, den, groups, den_groups, _, _ = sc.render_denoised_light_groups(rd, ROOM_GROUPS, ROOM_ENV_GROUP, albedo=albedo)
            rows = {"film": (sq_err(film, ref_film), sq_err(den, ref_film))}
            for g in range(3):
                rows["group %d" % g] = (sq_err(groups[g], ref_groups[g]), sq_err(den_groups[g], ref_groups[g]))
            for gains in GAINS:
                m = a.light_group_gains(gains)
                ref = lib.light_groups_mix(ref_groups, m)
                rows["relit %s" % (gains,)] = (sq_err(sc.light_groups_mix_resident(m), ref), sq_err(sc.light_groups_mix_resident(m, denoised=True), ref))
            sum_linf = float(np.abs(den_groups[..., :3].astype(np.float64).sum(axis=0) - den[..., :3].astype(np.float64)).max())
            key = "demodulated" if albedo else "plain"
            table[key] = {"rows": {k: {"noisy": n, "denoised": d, "ratio": d / n if n > 0 else None} for k, (n, d) in rows.items()},
                          "sum_of_denoised_groups_vs_denoised_film_linf": sum_linf, "denoised_film_max": float(den[..., :3].max())}
            for k, (n, d) in rows.items():
                if n > 0 and d / n > 1.0:
                    result["worse"].append({"size": size, "form": key, "row": k, "ratio": d / n})
        result["sizes"][str(size)] = table
    print(json.dumps(result))
    if args.out:
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
