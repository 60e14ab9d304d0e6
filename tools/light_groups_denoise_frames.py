#!/usr/bin/env python3
"""The frames of the adaptive and denoised light-group measurement: the Cornell box of C2 at `--size`² (max_bounces 8, L = 2) from one
process, after a warm-up, `--steps` alternating repeats, each call timed with the wall clock around it (every call ends in a synchronise).

  renders   pt_render and pt_render_light_groups at `--spp`; pt_render_adaptive and pt_render_adaptive_light_groups at G = 1, 3, 8 from `--spp` to
            `--max-samples` in steps of `--spp` at `--rel-error`.  `--parent-lib FILE` also times pt_render, pt_render_adaptive and pt_render_light_groups of
            another build of the engine (the parent commit's libptamd.so) in the same alternation and compares the films bit for bit.
  filter    per G: pt_denoise_light_groups_resident with every output read back, with none, and pt_denoise_light_groups of the host arrays; then the resident
            denoised mix.  The outputs are compared bit for bit.

Prints one JSON line: per part the median and the (min, max) of the repeats.  `--out FILE` writes the line's object to FILE.

`--trace CSV` is the kernel trace, a run of its own: per G a fresh child process of this file with `--kernels G` under rocprofv3 --kernel-trace --stats — pass
overlap off, one adaptive group render, `--steps` resident group filters, and for the yardstick one adaptive spectral render at bins = 4G (the same film) and
`--steps` resident quad filters (k_dn_gather_spectral_quad: the same 16-byte loads, with a transposition on either side) — and the kernels' rows are written to CSV.
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = (1, 3, 8)


def same(a, b):
    return bool(a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))


def trace(args):
    rows = []
    for G in GROUPS:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--kernels", str(G),
                   "--size", str(args.size), "--spp", str(args.spp), "--max-samples", str(args.max_samples), "--rel-error", str(args.rel_error), "--steps", str(args.steps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.trace_timeout)
            if r.returncode != 0:
                sys.exit("the traced run for G = %d ended with status %d\n%s" % (G, r.returncode, r.stderr[-2000:]))
            found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not found:
                sys.exit("rocprofv3 left no kernel_stats.csv for G = %d" % G)
            variant = ("tools/light_groups_denoise_frames.py --kernels %d (%dx%d Cornell box, %d..%d spp, rel_error %g, max_bounces 8, L = 2, PT_TUNE_NO_PASS_OVERLAP, %d filter "
                       "calls of each kind) under rocprofv3 --kernel-trace --stats: G = %d, bins = %d" % (G, args.size, args.size, args.spp, args.max_samples, args.rel_error,
                                                                                                             args.steps, G, 4 * G))
            for row in csv.DictReader(open(found[0])):
                rows.append([variant] + [row.get(k, "") for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")])
    with open(args.trace, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(["Variant", "Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs"])
        w.writerows(rows)
    print(json.dumps({"mode": "trace", "rows": len(rows), "csv": args.trace}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=250)
    ap.add_argument("--max-samples", type=int, default=500)
    ap.add_argument("--rel-error", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions of each call")
    ap.add_argument("--parent-lib", help="another build's libptamd.so: its renders are timed in the same alternation")
    ap.add_argument("--kernels", type=int, help="G: one render of each kind and the filters, without pass overlap, for a kernel trace")
    ap.add_argument("--trace", help="write the kernel trace's rows to this CSV (child processes under rocprofv3)")
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--out", help="write the result to this file")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
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
    ad = dict(max_samples=args.max_samples, rel_error=args.rel_error, step=args.spp)

    def adaptive_groups(s, G, desc=rd, read_groups=True, **kw):
        kw = kw or ad
        return s.render_adaptive_light_groups(desc, kw["max_samples"], kw["rel_error"], [0] * n_inst, G - 1, groups=G, step=kw["step"], stats=True, read_groups=read_groups)

    def warm_up(s):
        s.render(warm)
        s.render_adaptive(warm, 20, 0.1, step=10, stats=True)
        s.render_light_groups(warm, [0] * n_inst, 0, groups=1)
    warm_up(sc)
    for G in GROUPS:
        adaptive_groups(sc, G, desc=warm, max_samples=20, rel_error=0.1, step=10)
        if not args.kernels:   # (a trace counts every launch: the filters of a traced run are the timed ones alone)
            sc.resident_guides(warm, 4)
            sc.denoise_light_groups_resident()

    if args.kernels:
        G = args.kernels
        adaptive_groups(sc, G, read_groups=False)
        sc.resident_guides(rd, 4)
        for _ in range(args.steps):
            sc.denoise_light_groups_resident(film=False, groups=False)
        sc.render_adaptive_spectral(rd, 4 * G, ad["max_samples"], ad["rel_error"], step=ad["step"], stats=True)
        sc.resident_guides(rd, 4)
        for _ in range(args.steps):
            sc.denoise_resident(film=False)
        print(json.dumps({"mode": "kernels", "size": args.size, "G": G, "bins": 4 * G, "filter_calls": args.steps, "device": lib.device_info()}))
        return

    # (the three entries that exist in both builds run on scenes with one history — a scene of their own in this build too, which never sees a group filter or an
    # adaptive group render — so that the builds differ in nothing but their code)
    base = lib.create_scene(pkg.scene.cornell_box())
    warm_up(base)
    parent = a.Library(args.parent_lib).create_scene(pkg.scene.cornell_box()) if args.parent_lib else None
    if parent:
        warm_up(parent)
    parts = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        parts.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    plain = lambda s: s.render(rd)
    adaptive = lambda s: s.render_adaptive(rd, ad["max_samples"], ad["rel_error"], step=ad["step"], stats=True)
    grouped = lambda s: s.render_light_groups(rd, [0] * n_inst, 2, groups=3)
    plain(base); adaptive(base); grouped(base); adaptive_groups(sc, 8)   # warm-up at the timed size: the queues of the frame
    if parent:
        plain(parent); adaptive(parent); grouped(parent)
    bits = {}
    mean_count = None
    for _ in range(args.steps):
        film, _ = timed("pt_render", lambda: plain(base))
        afilm, counts, stats, _ = timed("pt_render_adaptive", lambda: adaptive(base))
        gfilm, groups, _ = timed("pt_render_light_groups_G3", lambda: grouped(base))
        mean_count = float(counts.mean())
        if parent:
            pfilm, _ = timed("pt_render_parent_build", lambda: plain(parent))
            pafilm, pcounts, pstats, _ = timed("pt_render_adaptive_parent_build", lambda: adaptive(parent))
            pgfilm, pgroups, _ = timed("pt_render_light_groups_G3_parent_build", lambda: grouped(parent))
            bits["pt_render_vs_parent_build"] = same(film, pfilm)
            bits["pt_render_adaptive_vs_parent_build"] = same(afilm, pafilm) and same(counts, pcounts) and same(stats, pstats)
            bits["pt_render_light_groups_vs_parent_build"] = same(gfilm, pgfilm) and same(groups, pgroups)
        for G in GROUPS:
            f, c, s, g, _ = timed("pt_render_adaptive_light_groups_G%d" % G, lambda: adaptive_groups(sc, G))
            bits["adaptive_groups_G%d_is_pt_render_adaptive" % G] = same(f, afilm) and same(c, counts) and same(s, stats)
    guides = lib.create_scene(pkg.scene.cornell_box()).render_guides(rd, 4)   # (the host-array call's: the bits resident_guides keeps on the device)
    for G in GROUPS:
        film, counts, stats, groups, _ = adaptive_groups(sc, G)
        sc.resident_guides(rd, 4)
        m = a.light_group_gains(np.linspace(0.5, 1.5, G))
        sc.denoise_light_groups_resident()   # warm-up: the first call at this size allocates the scene's buffers
        for _ in range(args.steps):
            res = timed("filter_resident_read_all_G%d" % G, lambda: sc.denoise_light_groups_resident())
            timed("filter_resident_read_nothing_G%d" % G, lambda: sc.denoise_light_groups_resident(film=False, groups=False))
            host = timed("filter_host_array_G%d" % G, lambda: lib.denoise_light_groups(film, counts, stats, guides, groups))
            relit = timed("mix_resident_denoised_G%d" % G, lambda: sc.light_groups_mix_resident(m, denoised=True))
        bits["filter_resident_vs_host_array_G%d" % G] = same(res[0], host[0]) and same(res[1], host[1])
        bits["mix_resident_denoised_vs_host_array_mix_G%d" % G] = same(relit, lib.light_groups_mix(host[1], m))
    summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
    result = {"size": args.size, "spp": args.spp, "max_samples": args.max_samples, "rel_error": args.rel_error, "mean_samples_per_pixel": mean_count, "steps": args.steps,
              "seconds": summary, "bit_for_bit": bits,
              "parent_lib": bool(parent), "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
