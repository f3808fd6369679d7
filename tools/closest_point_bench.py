#!/usr/bin/env python3
"""Closest-point query throughput on one GPU (rtamd.RayQuery.closest_point / rt_query_closest_point), outside
bench.py.

Method as tools/multihit_bench.py: teapot.scene at 1920x1080; after `--warmup` rounds, `--calls` timed rounds with one
call of every leg per round in a seeded shuffled order; HIP events on the calling stream, medians reported.  Legs:

  shell            2,073,600 points: the primary rays' hit positions (RayQuery.closest_hit) moved along the hit normal by
                   a seeded normal deviate of 1 % of the mesh's diagonal; row i takes the hit of the (i mod hits)-th
                   primary ray that hits something, with a deviate of its own (the number of hits is in the result).
                   The mesh is the triangles of material --mesh-material (0: in teapot.scene the two teapot meshes,
                   not the 2000-wide ground quad)
  shell_mesh       the same from the primary rays that hit the mesh itself (in teapot.scene most primary hits lie on the
                   ground quad, whose neighbourhood is two triangles)
  uniform          as many points uniform in the scene's triangle bounds (ground included) inflated by 25 %
  shell_maxdist, shell_mesh_maxdist
                   the shell points with max_dist = 1 % of the mesh's diagonal
  uniform_maxdist  the uniform points with the same max_dist
  closest          RayQuery.closest on the primary rays: the familiar yardstick

All four outputs are written in every closest-point leg.  After the timed rounds a second query object with the
counters build runs every closest-point leg once: mean nodes entered (Pn), internal nodes (Iv) and triangle tests (Tt)
per query, and the hit fraction.  Prints one JSON line and writes it to profiles/closest_point/closest_point_bench.json
(or --out).

    python tools/closest_point_bench.py [--calls 20] [--warmup 3] [--seed 1] [--scene teapot] [--out FILE]
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", default="teapot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mesh-material", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "closest_point", "closest_point_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("closest_point_bench: no HIP device")
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
        sys.exit("closest_point_bench: no triangle has material %d" % args.mesh_material)
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
            sys.exit("closest_point_bench: no primary ray hits the surface asked for")
        rows = rows[torch.arange(n, device=dev) % rows.numel()]
        step = 0.01 * diag * torch.randn((n, 1), generator=gen, device=dev)
        return (rec["position"][rows] + step * torch.nan_to_num(rec["normal"][rows])).contiguous()
    shell, shell_mesh = shell_of(rec["index"] >= 0), shell_of(on_mesh)
    max_dist = torch.full((n,), 0.01 * diag, dtype=torch.float32, device=dev)
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

    point_legs = {"shell": (shell, None), "shell_mesh": (shell_mesh, None), "uniform": (uniform, None),
                  "shell_maxdist": (shell, max_dist), "shell_mesh_maxdist": (shell_mesh, max_dist),
                  "uniform_maxdist": (uniform, max_dist)}
    legs = [(name, timed(lambda p=p, md=md: q.closest_point(p, md))) for name, (p, md) in point_legs.items()]
    legs.append(("closest", timed(lambda: q.closest(rays))))
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
    result = {"tool": "tools/closest_point_bench.py", "scene": args.scene, "width": args.width, "height": args.height,
              "calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "mesh_material": args.mesh_material, "mesh_triangles": int(tri.shape[0]), "mesh_diagonal": diag,
              "max_dist": 0.01 * diag, "primary_rays_that_hit": int((rec["index"] >= 0).sum()),
              "primary_rays_that_hit_the_mesh": int(on_mesh.sum()),
              "legs": {}}
    for name, _ in legs:
        ms = statistics.median(times[name])
        result["legs"][name] = {"queries": n, "event_ms_median": ms, "event_ms_min": min(times[name]),
                                "event_ms_max": max(times[name]), "mqueries_per_s_event": n / ms / 1e3}
    qc = rtamd.RayQuery(scene, counters=True)   # the counters build, a run of its own
    for name, (p, md) in point_legs.items():
        qc.closest_point(p, md, fields=())
        st = qc.stats()
        leg = result["legs"][name]
        leg["mean_nodes_entered"] = st["nodes_popped"] / n
        leg["mean_internal_nodes"] = st["internal_visits"] / n
        leg["mean_triangle_tests"] = st["triangle_tests"] / n
        leg["hit_fraction"] = st["hits"] / n
        leg["ratio_over_closest"] = leg["event_ms_median"] / result["legs"]["closest"]["event_ms_median"]
    qc.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
