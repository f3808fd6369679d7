#!/usr/bin/env python3
"""Cost of moving geometry under resident ray queries (rtamd.RayQuery.update / rt_query_update_triangles),
and what the frozen topology costs the queries afterwards.  Outside bench.py; nothing here is gated.

Per scene (teapot and lamp_available, the lamp meshes that ship, at 1920x1080), with the pixel-centre primary
rays of tools/query_bench.py and three vertex sets resident as torch tensors -- the scene's own vertices, a per-vertex jitter of 1 % of the scene
diagonal, and the mesh rotated rigidly by 30 degrees about the vertical axis through the root box's centre:

  update_<set>      RayQuery.update(vertices) on the device tensor: HIP events on the calling stream
  closest_<set>     RayQuery.closest on the primary rays with that set resident (the update before it untimed):
                    HIP events; Mrays/s before and after the deformations show how a refit tree degrades
  recreate_wall     the only alternative without the refit: destroy the object and create one from an edited
                    scene view (here a second Scene refitted on the host beforehand, so only destroy + create
                    are timed), on the wall clock, synchronised

`--warmup` rounds, then `--calls` timed rounds; every round runs each leg once in an order shuffled from the seed.
Medians and minima.  Prints one JSON line and writes it to profiles/refit/refit_bench.json (or --out).

    python tools/refit_bench.py [--calls 20] [--warmup 3] [--seed 1] [--scenes teapot,lamp_available] [--out FILE]
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

import torch   # before the library loads, so that both run on one HIP runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cuda-raytracer_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np   # noqa: E402
import rtamd   # noqa: E402
from query_bench import primary_rays   # noqa: E402


def vertex_sets(scene, seed):
    V = scene.vertices()
    root = scene.arrays()["bvh"][0]
    lo, hi = root[0:3].astype(np.float64), root[3:6].astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(seed)
    jitter = (V + (0.01 * diag) * rng.normal(size=V.shape)).astype(np.float32)
    c, a = (lo + hi) / 2, math.radians(30.0)
    rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    P = V.reshape(-1, 3).astype(np.float64)
    rotated = ((P - c) @ rot.T + c).astype(np.float32).reshape(-1, 9)
    return diag, {"original": V, "jitter": np.ascontiguousarray(jitter), "rotated": np.ascontiguousarray(rotated)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def bench_scene(name, args, dev):
    path = os.path.join(rtamd.ASSETS, name + ".scene")
    image = (args.width, args.height, 1, 1)
    scene = rtamd.Scene(path, image=image)
    diag, sets = vertex_sets(scene, args.seed)
    edited = rtamd.Scene(path, image=image)          # the edited host scene of the destroy + create alternative
    edited.refit(sets["jitter"])
    dsets = {k: torch.from_numpy(v).to(dev) for k, v in sets.items()}
    rays = primary_rays(scene, dev)
    n = rays.shape[0]
    q = rtamd.RayQuery(scene)
    q.reserve(n)
    q.update(dsets["original"])
    q.closest(rays)
    other = [rtamd.RayQuery(scene)]
    torch.cuda.synchronize()
    times = {}
    hits = {}

    def closest_leg(key):
        def run():
            ms, _ = timed(lambda: q.update(dsets[key]))
            times.setdefault("update_" + key, []).append(ms)
            ms, (t, index) = timed(lambda: q.closest(rays))
            hits[key] = float((index >= 0).float().mean())
            return "closest_" + key, ms
        return run

    def recreate():
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        other[0].close()
        other[0] = rtamd.RayQuery(edited)
        torch.cuda.synchronize()
        return "recreate_wall", (time.perf_counter() - w0) * 1e3

    legs = [closest_leg(k) for k in sets] + [recreate]
    shuffler = random.Random(args.seed)
    for k in range(args.warmup + args.calls):
        order = list(legs)
        shuffler.shuffle(order)
        if k == args.warmup:
            times.clear()
        for run in order:
            key, ms = run()
            times.setdefault(key, []).append(ms)
    # what the timed calls left resident is what the host twin computes
    q.update(dsets["jitter"])
    tri, bvh = q.geometry()
    arr = edited.arrays()
    same = bool(np.array_equal(tri.view(np.uint32), arr["triangles"].view(np.uint32)) and
                np.array_equal(bvh.view(np.uint32), arr["bvh"].view(np.uint32)))
    q.close()
    other[0].close()
    out = {"triangles": int(scene.view.triangle_count), "bvh_nodes": int(scene.view.bvh_node_count),
           "scene_diagonal": diag, "rays": n, "device_geometry_equals_host_refit": same, "hit_fraction": hits, "legs": {}}
    for key, v in sorted(times.items()):
        leg = {"samples": len(v), "ms_median": statistics.median(v), "ms_min": min(v)}
        if key.startswith("closest_"):
            leg["mrays_per_s"] = n / leg["ms_median"] / 1e3
        out["legs"][key] = leg
    upd = statistics.median([out["legs"]["update_" + k]["ms_median"] for k in sets])
    out["recreate_over_update"] = out["legs"]["recreate_wall"]["ms_median"] / upd
    for k in ("jitter", "rotated"):
        out["closest_slowdown_" + k] = out["legs"]["closest_" + k]["ms_median"] / out["legs"]["closest_original"]["ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scenes", default="teapot,lamp_available")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refit", "refit_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("refit_bench: no HIP device")
    import make_envmap
    make_envmap.ensure_envmap(os.path.join(REPO, "assets", "teapot", "textures", "envmap.pfm"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    result = {"tool": "tools/refit_bench.py", "width": args.width, "height": args.height, "calls": args.calls,
              "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0), "scenes": {}}
    for name in args.scenes.split(","):
        result["scenes"][name] = bench_scene(name, args, dev)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
