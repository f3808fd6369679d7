#!/usr/bin/env python3
"""Multi-hit query throughput on one GPU (rtamd.RayQuery.multi_hit / rt_query_multi_hit), outside bench.py.

Workload and method are tools/query_bench.py's: teapot.scene at 1920x1080, the 2,073,600 pixel-centre primary rays and
the cosine-distributed hemisphere rays from their triangle hit points (the same seed gives the same rays); after
`--warmup` rounds, `--calls` timed rounds with one call of every leg per round in a seeded shuffled order; HIP events on
the calling stream, medians reported.  Legs, on both ray sets (the hemisphere legs carry the suffix _hemi):

  multi_hit_k{1,4,16}        RayQuery.multi_hit with tmax = None
  multi_hit_k{1,4,16}_tmax   the same with tmax = 10 % of the scene diagonal
  occluded_any               RayQuery.occluded, tmax = None: the same traversal with the early exit
  occluded_tmax              the same at 10 % of the diagonal
  closest                    RayQuery.closest

For every multi-hit leg the result also has the mean count per ray and the cost relative to the occluded leg of the
same bound and to closest.  Prints one JSON line and writes it to profiles/multihit/multihit_bench.json (or --out).

    python tools/multihit_bench.py [--calls 20] [--warmup 3] [--seed 1] [--scene teapot] [--out FILE]
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
from query_bench import hemisphere_rays, primary_rays   # noqa: E402

KS = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", default="teapot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multihit", "multihit_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("multihit_bench: no HIP device")
    import make_envmap
    make_envmap.ensure_envmap(os.path.join(REPO, "assets", "teapot", "textures", "envmap.pfm"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    scene = rtamd.Scene(os.path.join(rtamd.ASSETS, args.scene + ".scene"), image=(args.width, args.height, 1, 1))
    arr = scene.arrays()
    root = arr["bvh"][0]
    diag = float(np.linalg.norm(root[3:6] - root[0:3]))
    q = rtamd.RayQuery(scene)
    rays = primary_rays(scene, dev)
    q.reserve(rays.shape[0])
    t, index = q.closest(rays)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    hemi = hemisphere_rays(rays, t, index, torch.from_numpy(arr["triangles"]).to(dev), scene.view.sphere_count, gen)
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

    legs = []
    for tag, r in (("", rays), ("_hemi", hemi)):
        n = r.shape[0]
        tmax = torch.full((n,), 0.1 * diag, dtype=torch.float32, device=dev)
        for k in KS:
            legs.append(("multi_hit_k%d%s" % (k, tag), n, timed(lambda r=r, k=k: q.multi_hit(r, k))))
            legs.append(("multi_hit_k%d_tmax%s" % (k, tag), n, timed(lambda r=r, k=k, tm=tmax: q.multi_hit(r, k, tm))))
        legs += [("occluded_any" + tag, n, timed(lambda r=r: q.occluded(r))),
                 ("occluded_tmax" + tag, n, timed(lambda r=r, tm=tmax: q.occluded(r, tm))),
                 ("closest" + tag, n, timed(lambda r=r: q.closest(r)))]
    times = {name: [] for name, _, _ in legs}
    shuffler = random.Random(args.seed)
    last = {}
    for rnd in range(args.warmup + args.calls):
        order = list(legs)                      # every leg once per round, in a seeded random order
        shuffler.shuffle(order)
        for name, _, run in order:
            ms, out = run()
            last[name] = out
            if rnd >= args.warmup:
                times[name].append(ms)
    result = {"tool": "tools/multihit_bench.py", "scene": args.scene, "width": args.width, "height": args.height,
              "calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "scene_diagonal": diag, "tmax": 0.1 * diag, "legs": {}}
    for name, n, _ in legs:
        ms = statistics.median(times[name])
        result["legs"][name] = {"rays": n, "event_ms_median": ms, "event_ms_min": min(times[name]),
                                "mrays_per_s_event": n / ms / 1e3}
    for tag in ("", "_hemi"):
        for k in KS:
            for bound, occ in (("", "occluded_any"), ("_tmax", "occluded_tmax")):
                name = "multi_hit_k%d%s%s" % (k, bound, tag)
                leg, count = result["legs"][name], last[name][2]
                leg["mean_count"] = float(count.float().mean())
                leg["max_count"] = int(count.max())
                leg["rows_truncated_fraction"] = float((count > k).float().mean())
                leg["ratio_over_occluded"] = leg["event_ms_median"] / result["legs"][occ + tag]["event_ms_median"]
                leg["ratio_over_closest"] = leg["event_ms_median"] / result["legs"]["closest" + tag]["event_ms_median"]
                # what the timed calls computed: count >= 1 <=> occluded with the same bound
                leg["count_ge1_equals_occluded"] = bool(torch.equal(count >= 1, last[occ + tag]))
    q.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
