"""CPU, world_size 2, backend gloo: the N > 1 path of the film sharding.  Each process renders its shard
with the emulated engine (tests/host_emulation — the product itself has no CPU path), the films are summed with one
`dist.reduce`, and the result must equal the single-process film bit for bit."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WORKER = r'''
import importlib, os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
pkg = importlib.import_module("rust-pathtracer_amd")
rank, local_rank, world = pkg.sharding.rank_world()
dist.init_process_group(backend="gloo", rank=rank, world_size=world)
emu = pkg.api.Library(os.path.join({here!r}, "host_emulation", "libptemu.so"), "ptemu_", optional=("render_device", "device_info"))
scene = emu.create_scene(pkg.scene.cornell_box())
S = pkg.sharding.weak_scaling_samples(3, world)
total = torch.zeros((40, 56, 4), dtype=torch.float32)
for k in range(2):
    rd = pkg.api.render_desc(56, 40, 2 * S, 4, tile=(16, 16), shard=pkg.sharding.shard(rank, world), first_sample=k * S, sample_count=S)
    film, prof = scene.render(rd)
    total += torch.from_numpy(film)
pkg.sharding.reduce_film(total, dst=0)
t = pkg.sharding.max_over_ranks(float(rank + 1), "cpu")
c = pkg.sharding.sum_over_ranks([prof.camera_rays], "cpu")
if rank == 0:
    np.save({out!r}, total.numpy())
    assert t == float(world) and c[0] == 56 * 40 * S, (t, c)
dist.destroy_process_group()
'''


import pytest  # noqa: E402


@pytest.mark.parametrize("world", [2, 8])
def test_n_process_gloo_reduce_equals_single_process(pkg, tmp_path, world):
    """(world = 8: the rank count of the driver's 8-GPU run — PT_TILE_SHARD(t, 8) across eight processes, the weak-scaling sample ranges, one reduce.)"""
    import emulation
    lib = emulation.library_path("ptemu")   # (the workers load it by this path)
    out = str(tmp_path / "film.npy")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, here=HERE, out=out))
    port = 29500 + (os.getpid() % 2000)
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port + world), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    reduced = np.load(out)
    emu = pkg.api.Library(lib, "ptemu_", optional=("render_device", "device_info"))
    scene = emu.create_scene(pkg.scene.cornell_box())
    S = pkg.sharding.weak_scaling_samples(3, world)
    whole = np.zeros_like(reduced)
    for k in range(2):
        film, _ = scene.render(pkg.api.render_desc(56, 40, 2 * S, 4, tile=(16, 16), first_sample=k * S, sample_count=S))
        whole += film
    assert np.array_equal(reduced, whole)


import json  # noqa: E402

import pytest  # noqa: E402


@pytest.mark.gpu
def test_bench_rccl_path_on_one_gpu(tmp_path):
    """bench.py --force-dist: torch.distributed with backend nccl (= RCCL) initialised for a single rank, so that the barrier, the film
    reduce and the max / sum over ranks of the N-GPU bench run through RCCL on the one GPU this box has.  The line must be the same
    kind of record as the plain run's."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 1000), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--spp-per-step", "16", "--cpu-seconds", "0"]
    lines = {}
    for tag, extra in (("dist", ["--force-dist", "--strong-legs", "--strong-spp-div", "64", "--strong-frames", "2"]), ("plain", []), ("strong", ["--scaling", "strong"])):
        r = subprocess.run(cmd + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip().splitlines()[-1].startswith('{"metric"'), r.stdout[-500:]   # the record is the last line of stdout
        lines[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    for tag, d in lines.items():
        assert d["n_gpus"] == 1 and d["value"] > 0 and d["config"]["samples_per_step"] == 1024 * 1024 * 16, tag
    assert lines["dist"]["segments_per_sample"] == lines["plain"]["segments_per_sample"]   # same paths, whoever sums the film
    for tag, d in lines.items():
        assert d["ranks_seen"] == 1 and d["physical_gpus"] == 1, tag
    assert lines["dist"]["backend"] == "nccl" and lines["dist"]["rccl_version"] and lines["plain"]["backend"] is None and lines["plain"]["strong"] is None
    # the fixed BASELINE frames as a leg of the same record (they always run with N > 1): C2 and C4, each with its clocks
    st = lines["dist"]["strong"]
    for leg, spp, L in (("C2", 1024 // 64, 2), ("C4", 2048 // 64, 6)):
        g = st[leg]
        assert g["n_gpus"] == 1 and g["frames"] == 2 and g["spp"] == spp and g["light_samples"] == L and g["samples_per_frame"] == 1024 * 1024 * spp, leg
        assert g["ms_per_frame"] > 0 and abs(g["value"] - g["samples_per_frame"] / (g["ms_per_frame"] * 1e-3) / 1e6) / g["value"] < 1e-6, leg
        assert 0 < g["reduce_ms"] < g["ms_per_frame"] and g["render_ms_fastest_rank"] <= g["render_ms_slowest_rank"] <= g["ms_per_frame"], leg
        assert g["setup_ms"] == g["setup"]["scene_create_ms"] + g["setup"]["first_frame_ms"] and g["film_bytes_reduced"] == 1024 * 1024 * 16, leg
        assert g["film_equals_one_rank"] is True and g["one_rank_check"]["ranks"] == 1 and g["rccl_ranks"] == 1 and g["backend"] == "nccl", leg
    # with one GPU the fixed-frame (strong scaling) run is the weak-scaling run: the same work, the same record but for the mode's name
    assert lines["strong"]["scaling"] == "strong" and lines["plain"]["scaling"] == "weak"
    for key in ("metric", "unit", "n_gpus", "steps", "segments_per_sample", "dtype"):
        assert lines["strong"][key] == lines["plain"][key], key
    assert lines["strong"]["config"]["workload_key"] == lines["plain"]["config"]["workload_key"]


GPU_WORKER = r'''
import importlib, os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
pkg = importlib.import_module("rust-pathtracer_amd")
rank, local_rank, world = pkg.sharding.rank_world()
dist.init_process_group(backend="gloo", rank=rank, world_size=world)
engine = pkg.load()                       # the real engine (libptamd.so): both processes on device 0
scene = engine.create_scene(pkg.scene.SCENES[{scene!r}]())
S = pkg.sharding.weak_scaling_samples(4, world)
total = torch.zeros(({h}, {w}, 4), dtype=torch.float32)
cam = 0
for k in range(2):
    rd = pkg.api.render_desc({w}, {h}, 2 * S, 6, light_samples=3, shard=pkg.sharding.shard(rank, world), first_sample=k * S, sample_count=S)
    film, prof = scene.render(rd)         # pt_render through the C ABI
    total += torch.from_numpy(film)
    cam += prof.camera_rays
pkg.sharding.reduce_film(total, dst=0)    # host reduce over gloo: the exchange step of the N-process path
c = pkg.sharding.sum_over_ranks([cam], "cpu")
if rank == 0:
    np.save({out!r}, total.numpy())
    assert c[0] == {w} * {h} * 2 * S, c
dist.destroy_process_group()
'''


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell_box", "hdri_small"])
def test_two_processes_on_one_gpu_equal_single_process(pkg, tmp_path, scene):
    """N > 1 with the real engine: two processes (gloo, world size 2), each rendering its shard of the film on device 0 with pt_render,
    the films summed on the host — and the result must equal the single-process film bit for bit (disjoint shards, RNG keyed by pixel)."""
    w, h = 232, 136
    out = str(tmp_path / "film.npy")
    script = tmp_path / "worker.py"
    script.write_text(GPU_WORKER.format(root=ROOT, here=HERE, out=out, scene=scene, w=w, h=h))
    port = 29700 + (os.getpid() % 1000)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    reduced = np.load(out)
    engine = pkg.load()
    sc = engine.create_scene(pkg.scene.SCENES[scene]())
    S = pkg.sharding.weak_scaling_samples(4, 2)
    whole = np.zeros_like(reduced)
    for k in range(2):
        film, _ = sc.render(pkg.api.render_desc(w, h, 2 * S, 6, light_samples=3, first_sample=k * S, sample_count=S))
        whole += film
    assert np.array_equal(reduced.view(np.uint32), whole.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 8])
def test_bench_gpus_n_launches_n_ranks(tmp_path, n):
    """(n = 8, round-4 verdict item 2: the shape of the driver's first 8-GPU run — eight ranks, PT_TILE_SHARD(..., 8) across processes, the weak steps at 8 x the
    samples, both strong legs at 1/8 of the frame per rank, one reduce per frame — rehearsed end to end on the one GPU, inside a stated wall-time budget.)
    `python bench.py --gpus 2` with no launcher around it: the parent (no GPU call) starts two ranks with torch.distributed.run and relays
    rank 0's record — n_gpus 2, ranks_seen 2 (all-reduced), strong-scaling legs included.  This box has one GPU and RCCL refuses two ranks on
    one device, so the ranks share it (--allow-shared-gpus, physical_gpus says so) and exchange over gloo; without the flag the run must stop."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    import time
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1", "--width", "256", "--height", "256", "--spp-per-step", "16",
           "--cpu-seconds", "0", "--backend", "gloo", "--strong-spp-div", "64", "--strong-frames", "2", "--full"]
    import torch
    if torch.cuda.device_count() < n:
        if n == 2:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            assert r.returncode != 0 and r.stdout.strip() == "" and ("has no GPU of its own" in r.stderr or "ranks on 1 physical GPU" in r.stderr), r.stderr[:3000]
        cmd.append("--allow-shared-gpus")
    t0 = time.time()
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    assert wall < 600, wall     # the budget: eight ranks that share ONE device and sixteen host threads set up, run the weak steps and both strong legs within ten minutes
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["ranks_seen"] == n and d["physical_gpus"] == min(n, torch.cuda.device_count()) and d["scaling"] == "weak" and "launched_by" in d
    assert d["config"]["spp_per_step"] == 16 * n and d["config"]["samples_per_step"] == 256 * 256 * 16 * n   # weak: 1/n of the pixels at n x the samples, per rank
    for leg, spp in (("C2", 16), ("C4", 32)):
        g = d["strong"][leg]
        assert g["n_gpus"] == n and g["samples_per_frame"] == 256 * 256 * spp and g["value"] > 0 and g["reduce_ms"] > 0, leg
        assert g["render_ms_slowest_rank"] >= g["render_ms_fastest_rank"] > 0, leg
        # the record checks SURVEY 8(e)'s claim itself: the n ranks' reduced film of a small frame against rank 0's own render of it, bit for bit, counters summed
        c = g["one_rank_check"]
        assert g["film_equals_one_rank"] is True and c["films_bitwise_equal"] and c["ranks"] == n and g["rccl_ranks"] == n, (leg, c)
        assert c["counters_n_ranks"] == c["counters_one_rank"] and c["counters_one_rank"][0] == 256 * 256 * spp and c["film_max"] > 0.0 and c["max_abs_difference"] == 0.0, (leg, c)
