#!/usr/bin/env python3
"""Host-path timings of the render entries on one GPU, for comparing two builds of the engine (PT_AMD_LIBRARY names the library; run the builds alternately):

  short_frame  256x256 Cornell box, 16 spp, max_bounces 4: `--calls` pt_render calls on one scene after `--warmup`, wall seconds per call (each call ends in its
               own synchronise and read-back) — the frame where the host's share is largest
  exchange     pt_render_spectral_multi, 1024x1024, B = 32, 120 spp, with one shard (PT_TUNE_MULTI_RCCL alone) and with multi_virtual = 4: the mean
               kernel_seconds[6] of `--frames` frames after one warm-up frame (the film reduce and the longest pack, copy and scatter)

Prints one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    pkg = importlib.import_module("rust-pathtracer_amd")
    lib = pkg.load()
    out = {"label": args.label, "library": pkg.LIBRARY_PATH}
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
