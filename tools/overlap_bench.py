#!/usr/bin/env python3
"""Box-overlap throughput on one GPU (rtamd.RayQuery.overlap_box / rt_query_overlap_box), outside bench.py.

Method as tools/nearest_k_bench.py: teapot.scene at 1920x1080; after `--warmup` rounds, `--calls` timed rounds with one
call of every leg per round in a seeded shuffled order; HIP events on the calling stream, medians reported.  Box centres
are closest_point_bench's point sets: shell (the primary rays' hit positions moved along the hit normal by a seeded normal
deviate of 1 % of the mesh's diagonal), shell_mesh (the same from the primary rays that hit the mesh itself) and uniform
(uniform in the scene's triangle bounds inflated by 25 %), 2,073,600 boxes each; the mesh is the triangles of material
--mesh-material.  Every box is a cube of half-extent 1 % of the mesh's diagonal.  Legs, per set:

  <set>_any        RayQuery.overlap_box, fields=("any",): the walk stops at a box's first member
  <set>_count      fields=("count",): the full walk, nothing kept
  <set>_k8, _k32   fields=("index", "count") with K = 8, 32
  <set>_nearest_k_count   what a caller did before: RayQuery.nearest_k, count only, at the box centre with max_dist = the
                   box's half-diagonal (the circumscribed sphere); its mean count over the box's is recorded

After the timed rounds a second query object with the counters build runs every leg once: mean count per query, mean nodes
entered (Pn), internal nodes (Iv) and triangle tests (Tt) per query, and the hit fraction.  Prints one JSON line and writes
it to profiles/overlap/overlap_bench.json (or --out).

    python tools/overlap_bench.py [--calls 10] [--warmup 3] [--seed 1] [--scene teapot] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch   # before the library loads, so that both run on one HIP runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cuda-raytracer_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np   # noqa: E402
import rtamd   # noqa: E402
from query_bench import primary_rays   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", default="teapot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mesh-material", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlap", "overlap_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("overlap_bench: no HIP device")
    import make_envmap
    make_envmap.ensure_envmap(os.path.join(REPO, "assets", "teapot", "textures", "envmap.pfm"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    scene = rtamd.Scene(os.path.join(rtamd.ASSETS, args.scene + ".scene"), image=(args.width, args.height, 1, 1))
    arr = scene.arrays()
    root = arr["bvh"][0]
    lo, hi = torch.from_numpy(root[0:3].copy()).to(dev), torch.from_numpy(root[3:6].copy()).to(dev)
    tri = arr["triangles"][arr["material_indices"][scene.view.sphere_count:] == args.mesh_material]
    if tri.shape[0] == 0:
        sys.exit("overlap_bench: no triangle has material %d" % args.mesh_material)
    verts = np.concatenate([tri[:, 0:3], tri[:, 0:3] + tri[:, 3:6], tri[:, 0:3] + tri[:, 6:9]])
    diag = float(np.linalg.norm(verts.max(0).astype(np.float64) - verts.min(0).astype(np.float64)))
    q = rtamd.RayQuery(scene)
    rays = primary_rays(scene, dev)
    n = rays.shape[0]
    q.reserve(n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    mid, half = (lo + hi) * 0.5, (hi - lo) * 0.5 * 1.25
    uniform = (mid + (torch.rand((n, 3), generator=gen, device=dev) * 2 - 1) * half).contiguous()
    rec = q.closest_hit(rays, fields=("index", "normal", "position", "material"))
    on_mesh = (rec["index"] >= scene.view.sphere_count) & (rec["material"] == args.mesh_material)

    def shell_of(mask):
        rows = torch.nonzero(mask).squeeze(1)
        if rows.numel() == 0:
            sys.exit("overlap_bench: no primary ray hits the surface asked for")
        rows = rows[torch.arange(n, device=dev) % rows.numel()]
        step = 0.01 * diag * torch.randn((n, 1), generator=gen, device=dev)
        return (rec["position"][rows] + step * torch.nan_to_num(rec["normal"][rows])).contiguous()
    centres = {"shell": shell_of(rec["index"] >= 0), "shell_mesh": shell_of(on_mesh), "uniform": uniform}
    h = 0.01 * diag
    boxes = {s: torch.cat([c - h, c + h], 1).contiguous() for s, c in centres.items()}
    max_dist = torch.full((n,), h * 3 ** 0.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), out
        return run

    modes = {"any": (1, ("any",)), "count": (1, ("count",)), "k8": (8, ("index", "count")), "k32": (32, ("index", "count")),
             "nearest_k_count": (1, None)}
    calls = {"%s_%s" % (s, m): (s, k, f) for s in centres for m, (k, f) in modes.items()}

    def call(obj, s, k, fields):
        if fields is None:
            return obj.nearest_k(centres[s], k, max_dist, fields=("count",))
        return obj.overlap_box(boxes[s], k, fields=fields)
    legs = [(name, timed(lambda a=a: call(q, *a))) for name, a in calls.items()]
    times = {name: [] for name, _ in legs}
    shuffler = random.Random(args.seed)
    for rnd in range(args.warmup + args.calls):
        order = list(legs)                      # every leg once per round, in a seeded random order
        shuffler.shuffle(order)
        for name, run in order:
            ms, _ = run()
            if rnd >= args.warmup:
                times[name].append(ms)
    q.close()
    result = {"tool": "tools/overlap_bench.py", "scene": args.scene, "width": args.width, "height": args.height,
              "calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "mesh_material": args.mesh_material, "mesh_triangles": int(tri.shape[0]), "mesh_diagonal": diag,
              "half_extent": h, "nearest_k_max_dist": h * 3 ** 0.5, "primary_rays_that_hit": int((rec["index"] >= 0).sum()),
              "primary_rays_that_hit_the_mesh": int(on_mesh.sum()), "legs": {}}
    for name, _ in legs:
        ms = statistics.median(times[name])
        result["legs"][name] = {"queries": n, "event_ms_median": ms, "event_ms_min": min(times[name]),
                                "event_ms_max": max(times[name]), "mqueries_per_s_event": n / ms / 1e3}
    qc = rtamd.RayQuery(scene, counters=True)   # the counters build, a run of its own
    for name, (s, k, fields) in calls.items():
        leg = result["legs"][name]
        out = call(qc, s, k, fields)
        if "count" in out:
            leg["mean_count"] = float(out["count"].double().mean())
        st = qc.stats()
        leg["mean_nodes_entered"] = st["nodes_popped"] / n
        leg["mean_internal_nodes"] = st["internal_visits"] / n
        leg["mean_triangle_tests"] = st["triangle_tests"] / n
        leg["hit_fraction"] = st["hits"] / n
    for s in centres:
        box, old = result["legs"][s + "_count"], result["legs"][s + "_nearest_k_count"]
        old["mean_count_over_box_count"] = old["mean_count"] / box["mean_count"] if box["mean_count"] else None
        old["event_ms_over_box_count"] = old["event_ms_median"] / box["event_ms_median"]
    qc.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
