#!/usr/bin/env python3
"""The frame of the development's measurement: the 1024x1024 Cornell box of C2 (tools/spectral_frames.py's frame, max_bounces 8,
L = 2) rendered once through pt_render_spectral at `--bins` bins, then developed `--steps` times with K = 3 (the colour-matching rows) and K = 9 responses,
through the resident entry and through the host-array entry.  Prints one JSON line with the mean whole-call seconds of each.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/spectral_project_frames.py --steps 1 --resident-only` for the per-dispatch times of
profiles/spectral_project_kernel_stats.csv: a run of its own, without counters.
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=120)
    ap.add_argument("--resident-only", action="store_true", help="skip the host-array entry (a kernel trace then holds the resident dispatches alone)")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    a = pkg.api
    sc = lib.create_scene(pkg.scene.cornell_box())
    rd = a.render_desc(args.size, args.size, args.spp, 8, seed=1)
    film, spectral, prof = sc.render_spectral(rd, args.bins)
    cie = lib.spectral_observer_matrix(rd, args.bins)
    nine = np.concatenate([cie, cie * np.float32(0.5), cie * np.float32(0.25)])
    out = {"bins": args.bins, "size": args.size, "spp": args.spp, "steps": args.steps, "render_seconds": prof.seconds}
    for name, matrix in (("K3", cie), ("K9", nine)):
        K = matrix.shape[0]
        bytes_moved = (args.bins + K) * args.size * args.size * 4
        sc.spectral_project_resident(matrix)   # (warm-up: the first call allocates the scene's development buffer)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = sc.spectral_project_resident(matrix)
        entry = {"K": K, "yardstick_bytes": bytes_moved, "resident_call_seconds": (time.perf_counter() - t0) / args.steps}
        if not args.resident_only:
            lib.spectral_project(spectral, matrix)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                host = lib.spectral_project(spectral, matrix)
            entry["host_array_call_seconds"] = (time.perf_counter() - t0) / args.steps
            entry["equal"] = bool(np.array_equal(res.view(np.uint32), host.view(np.uint32)))
        out[name] = entry
    y = sc.spectral_project_resident(cie)[1]
    out["mean_abs_Y_minus_film_Y"] = float(np.abs(y.astype(np.float64) - film[..., 1]).mean())
    out["mean_film_Y"] = float(film[..., 1].astype(np.float64).mean())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
