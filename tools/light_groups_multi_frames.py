#!/usr/bin/env python3
"""The frame of the group node entries' measurement ("On every device of a node"): the 1024x1024 Cornell box of C2 (max_bounces 8, L = 2)
at 120 spp with G = 1, 3 and 8 groups (the lamp in group 0, the environment in the last) on one GPU, rendered `--steps` times, the forms alternating, after
one warm-up frame of each:

  single     pt_render_light_groups
  one_shard  pt_render_light_groups_multi with PT_TUNE_MULTI_RCCL alone: the node path with one shard that is the whole film
  virtual4   pt_render_light_groups_multi with multi_virtual = 4: four shards on the one device, with kernel_seconds[6]

each timed with the wall clock around the whole call (every call ends in a synchronise; the group films are read back in all three).  Then, per G, the
node-resident mix (virtual4) against the one-device resident mix, `--mix-steps` times each; the assemble of an adaptive node group render (fixed count, with
statistics) against pt_resident_load of the film, counts and statistics it returned — the group films have no load form; and with `--parent-lib FILE`
pt_render_light_groups (G = 3) and pt_render of this build against another build of the engine (the parent commit's libptamd.so) in one process, alternating,
films compared bit for bit, beside this build's own run-to-run spread.

Prints one JSON line; `--out FILE` stores it under "frames" in FILE and leaves the file's other entries alone.  Nothing here measures more than one physical
device: on one GPU the node path gains nothing and is not meant to.

`--kernels` is the run for `rocprofv3 --kernel-trace --stats -- python3 tools/light_groups_multi_frames.py --kernels`: per G one virtual4 node render
(four k_light_groups_pack dispatches) and one adaptive node render with its assemble (four more, and four k_light_groups_unpack).
`--summarise TRACE.csv --csv OUT.csv` turns that run's kernel trace into the committed table: per G the pack and unpack dispatches at the timed size, their
bytes n_own * (4 + 32 G) and the ratio of the rate to 6.3 TB/s."""
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
FORMS = {"single": (0, False), "one_shard": (0, True), "virtual4": (4, False)}
STREAM_RATE = 6.3e12   # bytes per second a streaming kernel achieves on this GPU


def store(path, key, value):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    json.dump(data, open(path, "w"), indent=1)


def summarise(trace, out, size, shards):
    """The pack and unpack dispatches of a --kernels run: the warm-up's small grids apart, the run's order tells G (each G's dispatches come together)."""
    import csv
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    n_own = size * size // shards
    table = []
    for kernel in ("k_light_groups_pack", "k_light_groups_unpack"):
        mine = [r for r in rows if kernel in r["Kernel_Name"]]
        big = max([int(r["Grid_Size_X"]) for r in mine] or [0])
        mine = [r for r in mine if int(r["Grid_Size_X"]) == big]
        per_g = len(mine) // len(GROUPS) if mine else 0
        for k, G in enumerate(GROUPS):
            d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine[k * per_g:(k + 1) * per_g]]
            if not d:
                continue
            nbytes = n_own * (4 + 32 * G)
            avg = sum(d) / len(d)
            table.append([kernel, G, len(d), nbytes, "%.1f" % avg, min(d), max(d), "%.1f" % (nbytes / STREAM_RATE * 1e9), "%.2f" % (nbytes / (avg * 1e-9) / STREAM_RATE)])
    with open(out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(["Name", "Groups", "Calls", "BytesMoved", "AverageNs", "MinNs", "MaxNs", "YardstickNsAt6.3TBps", "RateOverYardstick"])
        w.writerows(table)
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=120)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions of each render")
    ap.add_argument("--mix-steps", type=int, default=10)
    ap.add_argument("--parent-lib", help="another build's libptamd.so: its pt_render_light_groups and pt_render are timed in the same alternation")
    ap.add_argument("--kernels", action="store_true", help="one node render and one assembled adaptive node render per G, for a kernel trace")
    ap.add_argument("--out", help="store the result in this JSON file")
    ap.add_argument("--summarise", help="a kernel trace CSV of a --kernels run")
    ap.add_argument("--csv", help="where --summarise writes its table")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.csv or "light_groups_multi_kernel_stats.csv", args.size, 4)
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    a = pkg.api
    n_inst = len(pkg.scene.cornell_box().instances)
    rd = a.render_desc(args.size, args.size, args.spp, 8, seed=1)
    warm = a.render_desc(64, 64, 10, 8, seed=1)
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)

    def scene(form, library=lib):
        virt, rccl = FORMS[form]
        t = library.tuning_default()
        t.multi_virtual = virt
        t.flags &= ~a.TUNE_MULTI_RCCL
        if rccl:
            t.flags |= a.TUNE_MULTI_RCCL
        return library.create_scene(pkg.scene.cornell_box(), t)

    def group_render(sc, form, G, desc=rd, read=True):
        if form == "single":
            return sc.render_light_groups(desc, [0] * n_inst, G - 1, groups=G, read_groups=read)
        return sc.render_light_groups_multi(desc, [0] * n_inst, G - 1, groups=G, read_groups=read, device_mask=1)

    def adaptive_node(sc, G, desc=rd):
        return sc.render_adaptive_light_groups_multi(desc, desc.spp, 0.0, [0] * n_inst, G - 1, groups=G, stats=True, device_mask=1)

    scenes = {form: scene(form) for form in FORMS}
    for form, sc in scenes.items():
        group_render(sc, form, 1, warm)   # warm-up: code objects, replicas, streams
    if args.kernels:
        sc = scenes["virtual4"]
        adaptive_node(sc, 1, a.render_desc(64, 64, 10, 8, seed=1))
        sc.resident_assemble()
        for G in GROUPS:
            group_render(sc, "virtual4", G)
            adaptive_node(sc, G)
            sc.resident_assemble()
        print(json.dumps({"mode": "kernels", "size": args.size, "spp": args.spp, "groups": GROUPS, "shards": 4,
                          "order": "per G a node render (4 packs), an adaptive node render (4 packs) and its assemble (4 unpacks)", "device": lib.device_info()}))
        return

    parts, checks = {}, {}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        parts.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    exchange = {}
    for form, sc in scenes.items():
        group_render(sc, form, 1)   # warm-up at the timed size: the queues of the frame
    for _ in range(args.steps):
        for G in GROUPS:
            got = {form: timed("%s_G%d" % (form, G), lambda: group_render(sc, form, G)) for form, sc in scenes.items()}
            exchange.setdefault(G, []).append(got["virtual4"][2].kernel_seconds[6])
            for form in ("one_shard", "virtual4"):
                checks["%s_G%d_equals_single" % (form, G)] = bool(np.array_equal(bits(got[form][0]), bits(got["single"][0])) and
                                                                  np.array_equal(bits(got[form][1]), bits(got["single"][1])))
    for G in GROUPS:
        M = np.random.default_rng(G).uniform(-2.0, 2.0, (G, 3, 3)).astype(np.float32)
        outs = {}
        for form in ("single", "virtual4"):
            sc = scenes[form]
            group_render(sc, form, G, read=False)
            sc.light_groups_mix_resident(M)   # warm-up: the first call allocates the scenes' buffers
            for _ in range(args.mix_steps):
                outs[form] = timed("mix_resident_%s_G%d" % (form, G), lambda: sc.light_groups_mix_resident(M))
        checks["mix_resident_G%d_equal" % G] = bool(np.array_equal(bits(outs["single"]), bits(outs["virtual4"])))
        sc = scenes["virtual4"]
        film, counts, st, groups, _ = adaptive_node(sc, G)
        sc.resident_assemble()   # warm-up: the first call allocates
        for _ in range(args.steps):
            timed("assemble_G%d" % G, lambda: sc.resident_assemble())
        back = sc.resident_read()
        checks["assembled_film_G%d_equal" % G] = bool(np.array_equal(bits(back[0]), bits(film)) and np.array_equal(back[1], counts))
        one = scenes["single"]
        one.resident_load(film=film, counts=counts, stats=st)
        for _ in range(args.steps):
            timed("resident_load_film_counts_stats", lambda: one.resident_load(film=film, counts=counts, stats=st))
    if args.parent_lib:
        plib = a.Library(args.parent_lib)
        mine, theirs = scene("single"), scene("single", plib)   # (two fresh scenes: neither carries the buffers of the renders above)
        for sc in (mine, theirs):
            sc.render_light_groups(rd, [0] * n_inst, 2, groups=3, read_groups=False)
            sc.render(rd)
        builds = [("this", mine), ("parent", theirs)]
        for step in range(args.steps):   # (the build that goes first changes from step to step: what runs behind what is shared out between the two)
            g, f = {}, {}
            for name, sc in builds if step % 2 == 0 else builds[::-1]:
                g[name] = timed("group_render_%s_build_G3" % name, lambda: sc.render_light_groups(rd, [0] * n_inst, 2, groups=3))
            for name, sc in builds if step % 2 == 0 else builds[::-1]:
                f[name] = timed("render_%s_build" % name, lambda: sc.render(rd))
            checks["group_render_vs_parent_build"] = bool(np.array_equal(bits(g["this"][0]), bits(g["parent"][0])) and np.array_equal(bits(g["this"][1]), bits(g["parent"][1])))
            checks["render_vs_parent_build"] = bool(np.array_equal(bits(f["this"][0]), bits(f["parent"][0])))
    summary = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in parts.items()}
    result = {"size": args.size, "spp": args.spp, "steps": args.steps, "mix_steps": args.mix_steps, "seconds": summary, "checks": checks,
              "virtual4_exchange_seconds": {"G%d" % G: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for G, v in exchange.items()},
              "pack_bytes_per_shard": {"G%d" % G: args.size * args.size // 4 * (4 + 32 * G) for G in GROUPS},
              "parent_lib": bool(args.parent_lib), "device": lib.device_info()}
    print(json.dumps(result))
    if args.out:
        store(args.out, "frames", result)


if __name__ == "__main__":
    main()
