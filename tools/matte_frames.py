#!/usr/bin/env python3
"""The frames of the ID-matte measurement: the 1024x1024 Cornell box and test_bokeh (82 instances behind a wide aperture: the top-level
walk) at S = 16 samples and R = 6 ranks.  Per scene, `--steps` times from one process after a warm-up, each timed with the wall clock around the call (every
call ends in a synchronise): pt_render_mattes without a read-back (the ranks stay on the device), pt_render_guides of the same S on the same build as the
yardstick — the same rays and probes with another fold — a resident extract of M = 4 selections, and the host-array extract of the same selections.

Prints one JSON line: per scene and part the median and the (min, max) of the repeats, and the checks (the resident extract equals the host-array one bit for
bit; sum of the coverage + overflow / S = 1).  `--out FILE` stores the line's object under "frames" in FILE and leaves the file's other entries alone.

Run it with `--kernels` under `rocprofv3 --kernel-trace --stats -- python3 tools/matte_frames.py --kernels` for the per-kernel times of
profiles/matte_kernel_stats.csv: a run of its own, per scene one matte render and `--extract-steps` resident extracts behind a warm-up at 64x64.
`--summarise TRACE.csv --csv OUT.csv` turns that run's kernel trace into the committed table: the fold, finish, extract, ray and probe kernels per scene, told
apart by the run's fixed order (the small grids of the warm-up are left out)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = ("cornell_box", "test_bokeh")
KERNELS = ("k_matte_fold", "k_matte_finish", "k_matte_extract", "k_probe_intersect", "k_guide_rays")


def store(path, key, value):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    json.dump(data, open(path, "w"), indent=1)


def summarise(trace, out):
    import csv
    import re
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = [r for r in rows if any(k in r["Kernel_Name"] for k in KERNELS)]
    # the probe's grid does not tell the warm-up from the frame, the rays' does: the first launch of k_guide_rays at the fold's large grid starts the first frame
    big = max(int(r["Grid_Size_X"]) for r in rows if "k_matte_fold" in r["Kernel_Name"])
    start = next(i for i, r in enumerate(rows) if "k_guide_rays" in r["Kernel_Name"] and int(r["Grid_Size_X"]) == big)
    groups, order, segment, extracted = {}, [], 0, False
    for r in rows[start:]:
        name = r["Kernel_Name"]
        short = re.search(r"(k_\w+(<[^>]*>)?)", name).group(1)
        if "k_matte_extract" in name:
            extracted = True
        elif extracted:   # (a render behind extracts: the next scene)
            segment, extracted = segment + 1, False
        key = (SCENES[segment] if segment < len(SCENES) else "segment %d" % segment, short)
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


def selections(keys):
    """M = 4: the most frequent object, every object, the sky, every second object and the sky."""
    present = [int(k) for k in np.unique(keys) if int(k) < 0xFFFFFFFE]
    first = max(present, key=lambda k: int((keys[0] == k).sum()))
    return [[first], present[:1023], [0xFFFFFFFE], present[::2][:1000] + [0xFFFFFFFE]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--ranks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5, help="timed repetitions of each call")
    ap.add_argument("--extract-steps", type=int, default=10)
    ap.add_argument("--kernels", action="store_true", help="per scene one matte render and the resident extracts, for a kernel trace")
    ap.add_argument("--out", help="store the result in this JSON file")
    ap.add_argument("--summarise", help="a kernel trace CSV of a --kernels run")
    ap.add_argument("--csv", help="where --summarise writes its table")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.csv or "matte_kernel_stats.csv")
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    a = pkg.api
    S, R = args.samples, args.ranks
    rd = a.render_desc(args.size, args.size, 10, 4, seed=1)
    warm = a.render_desc(64, 64, 10, 4, seed=1)
    result = {"size": args.size, "samples": S, "ranks": R, "steps": args.steps, "extract_steps": args.extract_steps, "device": lib.device_info(), "scenes": {}}
    scenes = {name: lib.create_scene(getattr(pkg.scene, name)()) for name in SCENES}
    for sc in scenes.values():   # warm-up: code objects, and in --kernels the segment the summary leaves out
        k, c, _ = sc.render_mattes(warm, S, ranks=R)
        sc.render_guides(warm, S)
        sc.matte_extract_resident(selections(k))
        lib.matte_extract(k, c, selections(k))
    for name, sc in scenes.items():
        if args.kernels:
            keys, _, _ = sc.render_mattes(rd, S, ranks=R)
            sel = selections(keys)
            for _ in range(args.extract_steps):
                sc.matte_extract_resident(sel)
            continue
        parts = {}

        def timed(part, fn):
            t0 = time.perf_counter()
            r = fn()
            parts.setdefault(part, []).append(time.perf_counter() - t0)
            return r

        keys, cov, over = sc.render_mattes(rd, S, ranks=R)   # warm-up at the timed size, and the planes of the host-array extract
        sc.render_guides(rd, S)
        sel = selections(keys)
        for _ in range(args.steps):
            timed("render_mattes", lambda: sc.render_mattes(rd, S, ranks=R, read=False))
            timed("render_mattes_read_back", lambda: sc.render_mattes(rd, S, ranks=R))
            timed("render_guides", lambda: sc.render_guides(rd, S))
        resident = sc.matte_extract_resident(sel)
        for _ in range(args.extract_steps):
            resident = timed("extract_resident_M4", lambda: sc.matte_extract_resident(sel))
            host = timed("extract_host_arrays_M4", lambda: lib.matte_extract(keys, cov, sel))
        counts = np.rint(cov.astype(np.float64) * S).astype(np.int64).sum(0) + over
        result["scenes"][name] = {
            "seconds": {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()},
            "distinct_keys": int(len(np.unique(keys[keys < 0xFFFFFFFE]))), "selected_keys": [len(s) for s in sel],
            "pixels_with_overflow": int((over > 0).sum()), "ranks_in_use": int((keys != 0xFFFFFFFF).any(axis=(1, 2)).sum()),
            "checks": {"resident_extract_equals_host_arrays": bool(resident.tobytes() == host.tobytes()), "counts_and_overflow_sum_to_S": bool((counts == S).all())}}
    if args.kernels:
        result["mode"] = "kernels"
        result["order"] = "a warm-up at 64x64 on both scenes, then per scene one matte render and its resident extracts"
    print(json.dumps(result))
    if args.out and not args.kernels:
        store(args.out, "frames", result)


if __name__ == "__main__":
    main()
