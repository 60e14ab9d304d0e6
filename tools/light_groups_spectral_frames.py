#!/usr/bin/env python3
"""The frames of the spectral light-group measurement: the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2, `--spp` samples, the
benchmark's 1024) through pt_render_light_groups and through pt_render_light_groups_spectral at G = 1, 4 and 8 (the lamp in group 0, the environment in the
last) and 8 and 32 bins, the renders alternating `--steps` times from one process after a warm-up, each timed with the wall clock around the call (every call
ends in a synchronise; the bins stay on the device).  `--parent-lib FILE` also times pt_render_light_groups of another build of the engine (the parent commit's
libptamd.so) in the same alternation, so that the two builds' group renders and the run-to-run spread come from one call.  Then the resident re-lamp at K = 3
against pt_spectral_project_resident at the same bins, `--relamp-steps` times each.

Prints one JSON line: per part the median and the (min, max) of the repeats and the films compared bit for bit.  `--out FILE` stores the line's object under
"frames" in FILE and leaves the file's other entries alone.

Run it with `--kernels` under `rocprofv3 --kernel-trace --stats -- python3 tools/light_groups_spectral_frames.py --kernels` for the per-kernel times of
profiles/light_groups_spectral_kernel_stats.csv: a run of its own, pass overlap off (PT_TUNE_NO_PASS_OVERLAP), one spectral render (k_accumulate_spectral), one
spectral group render per G and bin count (k_accumulate_group_bins) and `--relamp-steps` resident re-lamps and developments each.

`--summarise TRACE.csv --csv OUT.csv` turns that run's kernel trace into the committed table: the accumulate, development and re-lamp kernels per render of the run, told
apart by the run's fixed order.

`--resources` needs no GPU: registers, LDS and scratch of the new kernels from tools/resource_usage.py, stored under "resource_usage" with `--out`."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = (1, 4, 8)
BINS = (8, 32)


def store(path, key, value):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    json.dump(data, open(path, "w"), indent=1)


def summarise(trace, out):
    """The committed table from the kernel trace of a --kernels run.  The trace reports no dynamic LDS, so a launch's bin count is told by its place: the run
    renders in a fixed order and every render is followed by its developments or re-lamps, which end its segment."""
    import csv
    import re
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    configs = ["pt_render_spectral B=%d" % B for B in BINS] + ["pt_render_light_groups_spectral G=%d B=%d" % (G, B) for G in GROUPS for B in BINS]
    big = {k: max([int(r["Grid_Size_X"]) for r in rows if k in r["Kernel_Name"]] or [0]) for k in ("k_accumulate_group_bins", "k_accumulate_spectral")}
    # (the warm-up ends with a small spectral group render: everything up to its last k_accumulate_group_bins launch is left out)
    warm = [i for i, r in enumerate(rows) if "k_accumulate_group_bins" in r["Kernel_Name"] and int(r["Grid_Size_X"]) != big["k_accumulate_group_bins"]]
    rows = rows[warm[-1] + 1:] if warm else rows
    groups, order, segment, developed = {}, [], 0, False
    for r in rows:
        name = r["Kernel_Name"]
        m = re.search(r"(k_\w+(<[^>]*>)?)", name)
        short = m.group(1) if m else name
        develops = "k_light_groups_relamp" in name or "k_spectral_project" in name
        accumulates = any(k in name and int(r["Grid_Size_X"]) == big[k] for k in big)   # (the warm-up's small grids apart)
        if not develops and not accumulates:
            continue
        if accumulates and developed:
            segment, developed = segment + 1, False
        developed = developed or develops
        key = (configs[segment] if segment < len(configs) else "segment %d" % segment, short)
        if key not in groups:
            groups[key] = []
            order.append(key)
        groups[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(["Variant", "Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs"])
        for key in order:
            d = groups[key]
            w.writerow([key[0], key[1], len(d), sum(d), "%.1f" % (sum(d) / len(d)), min(d), max(d)])
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions of each render")
    ap.add_argument("--relamp-steps", type=int, default=10)
    ap.add_argument("--parent-lib", help="another build's libptamd.so: its pt_render_light_groups is timed in the same alternation")
    ap.add_argument("--kernels", action="store_true", help="one render of each kind, the re-lamps and the developments, without pass overlap, for a kernel trace")
    ap.add_argument("--resources", action="store_true", help="the new kernels' registers, LDS and scratch (no GPU)")
    ap.add_argument("--out", help="store the result in this JSON file")
    ap.add_argument("--summarise", help="a kernel trace CSV of a --kernels run")
    ap.add_argument("--csv", help="where --summarise writes its table")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.csv or "light_groups_spectral_kernel_stats.csv")
    if args.resources:
        text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "pt_light_groups_spectral.hip"], capture_output=True, text=True, check=True).stdout
        rows = []
        for line in text.strip().split("\n")[1:]:
            f = line.split()
            rows.append({"kernel": f[0], "vgpr": int(f[1]), "agpr": int(f[2]), "sgpr": int(f[3]), "scratch_bytes": int(f[4]), "static_lds_bytes": int(f[8]),
                         "dynamic_lds_bytes": "256 * bins * 4 (at most 65536)" if f[0] == "k_accumulate_group_bins" else 0})
        print(json.dumps(rows))
        if args.out:
            store(args.out, "resource_usage", rows)
        return
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

    def group_render(scene, G, desc=rd):
        return scene.render_light_groups(desc, [0] * n_inst, G - 1, groups=G, read_groups=False)

    def spectral_group_render(G, B, desc=rd):
        return sc.render_light_groups_spectral(desc, B, [0] * n_inst, G - 1, groups=G, read_groups=False, read_bins=False)

    def matrices(G, B):
        R = lib.spectral_observer_matrix(rd, B)
        return R, np.ascontiguousarray(np.repeat(R[:, None, :], G, axis=1))

    sc.render(warm)
    for G in GROUPS:
        group_render(sc, G, warm)
        spectral_group_render(G, 8, warm)   # warm-up: code objects
    if args.kernels:
        for B in BINS:
            sc.render_spectral(rd, B)
            R, _ = matrices(1, B)
            for _ in range(args.relamp_steps):
                sc.spectral_project_resident(R)
        for G in GROUPS:
            for B in BINS:
                spectral_group_render(G, B)
                _, W = matrices(G, B)
                for _ in range(args.relamp_steps):
                    sc.light_groups_relamp_resident(W)
        print(json.dumps({"mode": "kernels", "size": args.size, "spp": args.spp, "groups": GROUPS, "bins": BINS, "relamp_calls_each": args.relamp_steps,
                          "order": "per bin count a spectral render and its developments, then per G and bin count a spectral group render and its re-lamps",
                          "device": lib.device_info()}))
        return

    parent = a.Library(args.parent_lib).create_scene(pkg.scene.cornell_box()) if args.parent_lib else None
    if parent:
        group_render(parent, 1, warm)
    parts = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        parts.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    group_render(sc, 1)   # warm-up at the timed size: the queues of the frame
    same = {}
    for _ in range(args.steps):
        for G in GROUPS:
            film, _, _ = timed("group_render_G%d" % G, lambda: group_render(sc, G))
            if parent:
                pfilm, _, _ = timed("group_render_parent_build_G%d" % G, lambda: group_render(parent, G))
                same["group_render_vs_parent_build_G%d" % G] = bool(np.array_equal(film.view(np.uint32), pfilm.view(np.uint32)))
            for B in BINS:
                sfilm = timed("spectral_group_render_G%d_B%d" % (G, B), lambda: spectral_group_render(G, B))[0]
                same["film_G%d_B%d" % (G, B)] = bool(np.array_equal(film.view(np.uint32), sfilm.view(np.uint32)))
    for B in BINS:
        sc.render_spectral(rd, B)
        R, _ = matrices(1, B)
        sc.spectral_project_resident(R)   # warm-up: the first call allocates the scene's buffer
        for _ in range(args.relamp_steps):
            timed("project_resident_B%d" % B, lambda: sc.spectral_project_resident(R))
        for G in GROUPS:
            spectral_group_render(G, B)
            _, W = matrices(G, B)
            out = sc.light_groups_relamp_resident(W)
            for _ in range(args.relamp_steps):
                out = timed("relamp_resident_G%d_B%d" % (G, B), lambda: sc.light_groups_relamp_resident(W))
            same["relamp_finite_G%d_B%d" % (G, B)] = bool(np.isfinite(out).all())
    summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
    result = {"size": args.size, "spp": args.spp, "steps": args.steps, "relamp_steps": args.relamp_steps, "seconds": summary, "checks": same,
              "parent_lib": bool(parent), "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        store(args.out, "frames", result)


if __name__ == "__main__":
    main()
