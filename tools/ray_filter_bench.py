#!/usr/bin/env python3
"""Filtered ray-query throughput on one GPU (rtamd.RayQuery.closest_filtered / occluded_filtered), outside
bench.py.

Method as tools/query_bench.py and the other query benches: teapot.scene at 1920x1080; after `--warmup` rounds,
`--calls` timed rounds with one call of every leg per round in a seeded shuffled order; HIP events on the calling
stream, medians reported.  Legs on the primary rays (pixel centres, 2,073,600):

  closest             RayQuery.closest: the yardstick leg (the reference's far-child-first walk)
  filtered_empty      closest_filtered with no filter and no masks: the near-child-first walk on the same rays
  filtered_masked     closest_filtered with primitive masks (one bit per material) and a ray mask that hides the ground
                      plane's material (--hide-material; by default the material most primary rays hit)
  filtered_interval   closest_filtered with tmin = 0.5 and tmax = 1.5 times the median primary hit distance

and on the hemisphere rays of tools/query_bench.py (from the primary rays' triangle hits):

  closest_hemi        RayQuery.closest
  filtered_hemi_skip  closest_filtered with skip = the triangle the ray starts on
  occluded_hemi       RayQuery.occluded
  occluded_filtered_hemi_empty, occluded_filtered_hemi_masked   occluded_filtered, no filter / the masks above

After the timed rounds a second query object with the counters build runs every leg once: nodes entered (Pn), internal
nodes (Iv) and triangle tests (Tt) per ray, and the hit fraction.  Prints one JSON line and writes it to
profiles/ray_filter/ray_filter_bench.json (or --out).

    python tools/ray_filter_bench.py [--calls 20] [--warmup 3] [--seed 1] [--scene teapot] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", default="teapot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--hide-material", type=int, default=-1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ray_filter", "ray_filter_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("ray_filter_bench: no HIP device")
    import make_envmap
    make_envmap.ensure_envmap(os.path.join(REPO, "assets", "teapot", "textures", "envmap.pfm"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    scene = rtamd.Scene(os.path.join(rtamd.ASSETS, args.scene + ".scene"), image=(args.width, args.height, 1, 1))
    arr = scene.arrays()
    S = scene.view.sphere_count
    q = rtamd.RayQuery(scene)
    rays = primary_rays(scene, dev)
    n = rays.shape[0]
    q.reserve(n)
    rec = q.closest_hit(rays, fields=("t", "index", "material"))
    hit = rec["index"] >= 0
    if not bool(hit.any()):
        sys.exit("ray_filter_bench: no primary ray hits anything")
    hide = args.hide_material
    if hide < 0:
        hide = int(torch.bincount(rec["material"][hit].long()).argmax())
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    hemi = hemisphere_rays(rays, rec["t"], rec["index"], torch.from_numpy(arr["triangles"]).to(dev), S, gen)
    start = rec["index"][rec["index"] >= S].contiguous()          # the triangle each hemisphere ray starts on
    nh = hemi.shape[0]
    med = float(rec["t"][hit].median())
    table = np.left_shift(np.uint32(1), (np.arange(scene.view.material_count) % 32).astype(np.uint32)).astype(np.uint32)
    masks = torch.from_numpy(rtamd.masks_from_materials(scene, table).view(np.int32)).to(dev)
    hide_word = int(np.array([~table[hide]], np.uint32).view(np.int32)[0])
    see = {m: torch.full((m,), hide_word, dtype=torch.int32, device=dev) for m in (n, nh)}
    tmin = torch.full((n,), 0.5 * med, dtype=torch.float32, device=dev)
    tmax = torch.full((n,), 1.5 * med, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    # leg -> (rays of the leg, whether the object holds the masks, the call on a query object)
    calls = {
        "closest": (n, False, lambda o: o.closest(rays)),
        "filtered_empty": (n, False, lambda o: o.closest_filtered(rays)),
        "filtered_masked": (n, True, lambda o: o.closest_filtered(rays, mask=see[n])),
        "filtered_interval": (n, False, lambda o: o.closest_filtered(rays, tmin=tmin, tmax=tmax)),
        "closest_hemi": (nh, False, lambda o: o.closest(hemi)),
        "filtered_hemi_skip": (nh, False, lambda o: o.closest_filtered(hemi, skip=start)),
        "occluded_hemi": (nh, False, lambda o: o.occluded(hemi)),
        "occluded_filtered_hemi_empty": (nh, False, lambda o: o.occluded_filtered(hemi)),
        "occluded_filtered_hemi_masked": (nh, True, lambda o: o.occluded_filtered(hemi, mask=see[nh])),
    }

    def run(obj, name):
        count, masked, fn = calls[name]
        obj.set_masks(masks if masked else None)       # outside the timed span
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(obj)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    times = {name: [] for name in calls}
    shuffler = random.Random(args.seed)
    for rnd in range(args.warmup + args.calls):
        order = list(calls)                            # every leg once per round, in a seeded random order
        shuffler.shuffle(order)
        for name in order:
            ms, _ = run(q, name)
            if rnd >= args.warmup:
                times[name].append(ms)
    q.close()
    result = {"tool": "tools/ray_filter_bench.py", "scene": args.scene, "width": args.width, "height": args.height,
              "calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "primary_rays": n, "hemisphere_rays": nh, "hidden_material": hide, "median_primary_t": med, "legs": {}}
    for name, (count, _, _) in calls.items():
        ms = statistics.median(times[name])
        result["legs"][name] = {"rays": count, "event_ms_median": ms, "event_ms_min": min(times[name]),
                                "event_ms_max": max(times[name]), "mrays_per_s_event": count / ms / 1e3}
    qc = rtamd.RayQuery(scene, counters=True)          # the counters build, a run of its own
    for name, (count, _, _) in calls.items():
        run(qc, name)
        st = qc.stats()
        leg = result["legs"][name]
        leg["nodes_entered_per_ray"] = st["nodes_popped"] / count
        leg["internal_nodes_per_ray"] = st["internal_visits"] / count
        leg["triangle_tests_per_ray"] = st["triangle_tests"] / count
        leg["hit_fraction"] = st["hits"] / count
    qc.close()
    for name, leg in result["legs"].items():
        if name.startswith("occluded"):
            yard = "occluded_hemi"
        else:
            yard = "closest_hemi" if "hemi" in name else "closest"
        leg["ratio_over_" + yard] = leg["event_ms_median"] / result["legs"][yard]["event_ms_median"]
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
