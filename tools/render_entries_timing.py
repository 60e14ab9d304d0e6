#!/usr/bin/env python3
"""Host-path timings of the render entries on one GPU, for comparing two builds of the engine (PT_AMD_LIBRARY names the library; run the builds alternately):

  short_frame  256x256 Cornell box, 16 spp, max_bounces 4: `--calls` pt_render calls on one scene after `--warmup`, wall seconds per call (each call ends in its
               own synchronise and read-back) — the frame where the host's share is largest
  exchange     pt_render_spectral_multi, 1024x1024, B = 32, 120 spp, with one shard (PT_TUNE_MULTI_RCCL alone) and with multi_virtual = 4: the mean
               kernel_seconds[6] of `--frames` frames after one warm-up frame (the film reduce and the longest pack, copy and scatter)
  --entries    instead of the two above: the entries around a film at `--size` squared, `--bins` bins, 4 guide samples (the *_frames.py scripts' sizes) on the
               glass-slab scene — the guide pass at the first hit and with a chain of 8, alone and with both albedos, host-array and resident; the matte
               render (16 samples, 6 ranks) and the resident extract of matte_frames.py's 4 selections; the resident development, mix and re-lamp (G = 4,
               K = 3); both resident filters with nothing read back.  Per entry the median wall seconds of `--steps` calls after one warm-up call.

Prints one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import timeit

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def entries(pkg, lib, size, bins, steps):
    a = pkg.api
    from matte_frames import selections
    builder = pkg.scene.cornell_checker_slab()
    groups = ([0] * len(builder.instances), 3)   # G = 4: the emitters in group 0, the environment in group 3
    sc = lib.create_scene(builder)
    rd = a.render_desc(size, size, 10, 8, seed=1)
    seconds = {}

    def timed(name, call):
        call()
        seconds[name] = statistics.median(timeit.repeat(call, number=1, repeat=steps))

    sc.render_adaptive_spectral(rd, bins, 20, 0.05, stats=True)   # (few samples: the entries' work does not depend on the film's values)
    for chain in (0, 8):
        timed("guides_host_chain%d" % chain, lambda: sc.render_guides_chain(rd, 4, chain, albedo=False) if chain else sc.render_guides(rd, 4))
        timed("guides_albedos_host_chain%d" % chain, lambda: sc.render_guides_bin_albedo(rd, bins, 4, chain))
        timed("guides_resident_chain%d" % chain, lambda: sc.resident_guides(rd, 4, specular_chain=chain))
        timed("guides_albedos_resident_chain%d" % chain, lambda: sc.resident_guides(rd, 4, specular_chain=chain, albedo=True, bin_albedo=True))
    timed("denoise_resident", lambda: sc.denoise_resident(film=False))
    M = lib.spectral_observer_matrix(rd, bins)
    timed("spectral_project_resident", lambda: sc.spectral_project_resident(M))
    keys, _, _ = sc.render_mattes(rd, 16, ranks=6)
    timed("render_mattes", lambda: sc.render_mattes(rd, 16, ranks=6, read=False))
    sel = selections(keys)
    timed("matte_extract_resident", lambda: sc.matte_extract_resident(sel))
    sc.render_adaptive_light_groups(rd, 20, 0.05, *groups, groups=4, read_groups=False)
    sc.resident_guides(rd, 4, albedo=True)
    timed("denoise_light_groups_resident", lambda: sc.denoise_light_groups_resident(film=False, groups=False))
    mix = np.ascontiguousarray(np.tile(np.eye(3, dtype=np.float32), (4, 1, 1)))
    timed("light_groups_mix_resident", lambda: sc.light_groups_mix_resident(mix))
    sc.render_light_groups_spectral(rd, bins, *groups, groups=4, read_groups=False, read_bins=False)
    relamp = np.ascontiguousarray(np.repeat(M[:, None, :], 4, axis=1))
    timed("light_groups_relamp_resident", lambda: sc.light_groups_relamp_resident(relamp))
    sc.close()
    return seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", action="store_true")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    out = {"label": args.label, "library": pkg.LIBRARY_PATH}
    if args.entries:
        out.update(size=args.size, bins=args.bins, steps=args.steps, entries_median_seconds=entries(pkg, lib, args.size, args.bins, args.steps))
        print(json.dumps(out), flush=True)
        return
    sc = lib.create_scene(pkg.scene.cornell_box())
    rd = pkg.api.render_desc(256, 256, 16, 4, seed=1)
    for _ in range(args.warmup):
        sc.render(rd)
    per_call = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        sc.render(rd)
        per_call.append(time.perf_counter() - t0)
    sc.close()
    out["short_frame_calls"] = args.calls
    out["short_frame_mean_seconds"] = statistics.fmean(per_call)
    out["short_frame_median_seconds"] = statistics.median(per_call)
    rd = pkg.api.render_desc(1024, 1024, 120, 8, seed=1)
    for form, virt in (("one_shard", 0), ("virtual4", 4)):
        t = lib.tuning_default()
        t.multi_virtual = virt
        t.flags |= pkg.api.TUNE_MULTI_RCCL
        sc = lib.create_scene(pkg.scene.cornell_box(), t)
        sc.render_spectral_multi(rd, 32, device_mask=1)
        profs = [sc.render_spectral_multi(rd, 32, device_mask=1)[-1] for _ in range(args.frames)]
        sc.close()
        out["exchange_%s_seconds" % form] = statistics.fmean(p.kernel_seconds[6] for p in profs)
        out["exchange_%s_frames" % form] = [p.kernel_seconds[6] for p in profs]
        out["frame_%s_seconds" % form] = statistics.fmean(p.seconds for p in profs)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
