#!/usr/bin/env python3
"""Hemisphere-query throughput on one GPU (rtamd.RayQuery.hemisphere), outside bench.py.

Method as tools/ray_filter_bench.py: teapot.scene at 1920x1080; the frames are the primary rays' triangle hits (the hit
point, the triangle's normal turned against the ray), skip = the hit triangle.  For every S of --samples: after
`--warmup` rounds, `--calls` timed rounds with one call of every leg per round in a seeded shuffled order; HIP events on
the calling stream, medians reported.  Legs:

  fused     RayQuery.hemisphere(points, normals, S, skip=...): the rays are made on the device, one int per point comes back
  composed  what a caller had to write before: n * S cosine rays made in torch as tools/query_bench.py makes them (inside
            the timed span), occluded_filtered with skip, reshape and sum
  floor     occluded_filtered alone on rays made beforehand: the traversal

composed and floor need the n * S rays in device memory (24 B each, the library's 48 B of scratch and torch's temporaries
on top); where they do not fit (--ray-bytes per ray against the free memory, or an allocation failure) the leg says so.
After the timed rounds a second query object with the counters build runs the fused call once per S: nodes entered,
internal nodes and triangle tests per sample, and the open fraction.  Prints one JSON line and writes it to
profiles/hemisphere/hemisphere_bench.json (or --out).

    python tools/hemisphere_bench.py [--samples 1,16,64,256] [--calls 20] [--warmup 3] [--legs fused,composed,floor]
                                     [--points N] [--seed 1] [--scene teapot] [--out FILE]
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
import rtamd   # noqa: E402
from query_bench import primary_rays, unit   # noqa: E402


def cosine_rays(p, n, samples, gen):
    """n * S rays in torch: origin = the point, direction cosine-distributed about the normal (query_bench's form)."""
    p, n = p.repeat_interleave(samples, 0), n.repeat_interleave(samples, 0)
    u = torch.rand((p.shape[0], 2), generator=gen, device=p.device, dtype=torch.float32)
    rad, phi = u[:, :1].sqrt(), 2 * torch.pi * u[:, 1:]
    helper = torch.where(n[:, :1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device=p.device),
                         torch.tensor([0.0, 1.0, 0.0], device=p.device))
    bx = unit(torch.linalg.cross(n, helper))
    by = torch.linalg.cross(n, bx)
    w = unit(rad * phi.cos() * bx + rad * phi.sin() * by + (1 - u[:, :1]).clamp_min(0).sqrt() * n)
    return torch.cat([p, w], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1,16,64,256")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="fused,composed,floor")
    ap.add_argument("--points", type=int, default=0, help="use only the first N frames (0 = all)")
    ap.add_argument("--ray-bytes", type=int, default=260, help="device bytes per sample ray the composed path is assumed to need")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", default="teapot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hemisphere", "hemisphere_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    legs = [x for x in args.legs.split(",") if x]
    if not legs or set(legs) - {"fused", "composed", "floor"}:
        ap.error("--legs: fused, composed, floor")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("hemisphere_bench: no HIP device")
    import make_envmap
    make_envmap.ensure_envmap(os.path.join(REPO, "assets", "teapot", "textures", "envmap.pfm"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    scene = rtamd.Scene(os.path.join(rtamd.ASSETS, args.scene + ".scene"), image=(args.width, args.height, 1, 1))
    S0 = scene.view.sphere_count
    q = rtamd.RayQuery(scene)
    rays = primary_rays(scene, dev)
    rec = q.closest_hit(rays, fields=("t", "index", "position"))
    keep = rec["index"] >= S0
    if not bool(keep.any()):
        sys.exit("hemisphere_bench: no primary ray hits a triangle")
    tris = torch.from_numpy(scene.arrays()["triangles"]).to(dev)
    skip = rec["index"][keep].contiguous()
    pts = rec["position"][keep].contiguous()
    nrm = tris[(skip - S0).long(), 9:12]
    nrm = torch.where((nrm * rays[keep][:, 3:]).sum(1, keepdim=True) > 0, -nrm, nrm).contiguous()
    if args.points:
        pts, nrm, skip = pts[:args.points].contiguous(), nrm[:args.points].contiguous(), skip[:args.points].contiguous()
    n = pts.shape[0]
    del rays, rec
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    shuffler = random.Random(args.seed)
    result = {"tool": "tools/hemisphere_bench.py", "scene": args.scene, "width": args.width, "height": args.height,
              "calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "library": os.path.basename(os.path.dirname(rtamd.LIB_PATH)) + "/" + os.path.basename(rtamd.LIB_PATH),
              "points": n, "scratch_bytes_per_point": 44, "composed_bytes_per_sample_at_least": 65, "samples": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for S in [int(x) for x in args.samples.split(",")]:
        total = n * S
        entry = {"sample_rays": total, "legs": {}}
        result["samples"][str(S)] = entry
        per_ray_skip = pre = None
        skipped = {}
        todo = list(legs)
        if "composed" in todo or "floor" in todo:
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info()[0]
            if total > 0x7FFFFFFF:
                why = "n * S = %d rays exceed one call's int32 ray count" % total
            elif total * args.ray_bytes > free:
                why = "n * S = %d rays at ~%d B each do not fit in %.1f GB of free device memory" % (total, args.ray_bytes, free / 1e9)
            else:
                why = None
                try:
                    per_ray_skip = skip.repeat_interleave(S).contiguous()
                    if "floor" in todo:
                        pre = cosine_rays(pts, nrm, S, gen)
                    q.reserve(total)
                except (RuntimeError, rtamd.RtError) as e:
                    why = "allocation failed: %s" % str(e).splitlines()[0]
                    per_ray_skip = pre = None
                    torch.cuda.empty_cache()
            if why:
                for leg in ("composed", "floor"):
                    if leg in todo:
                        todo.remove(leg)
                        skipped[leg] = why

        def fused():
            return q.hemisphere(pts, nrm, S, "cosine", seed=args.seed, skip=skip, fields=("open_count",))["open_count"]

        def composed():
            r = cosine_rays(pts, nrm, S, gen)
            occ = q.occluded_filtered(r, skip=per_ray_skip)
            return S - occ.view(n, S).sum(1, dtype=torch.int32)

        def floor():
            return q.occluded_filtered(pre, skip=per_ray_skip)

        fns = {"fused": fused, "composed": composed, "floor": floor}
        times = {leg: [] for leg in todo}
        for rnd in range(args.warmup + args.calls):
            order = list(todo)
            shuffler.shuffle(order)
            for leg in order:
                ms, _ = timed(fns[leg])
                if rnd >= args.warmup:
                    times[leg].append(ms)
        for leg in todo:
            ms = statistics.median(times[leg])
            entry["legs"][leg] = {"event_ms_median": ms, "event_ms_min": min(times[leg]), "event_ms_max": max(times[leg]),
                                  "msamples_per_s": total / ms / 1e3}
        for leg, why in skipped.items():
            entry["legs"][leg] = {"skipped": why}
        if "fused" in entry["legs"]:
            for leg in ("composed", "floor"):
                if leg in times:
                    entry["legs"]["fused"]["time_over_" + leg] = (entry["legs"]["fused"]["event_ms_median"] /
                                                                  entry["legs"][leg]["event_ms_median"])
        del pre, per_ray_skip
        torch.cuda.empty_cache()
    q.close()
    if "fused" in legs:
        qc = rtamd.RayQuery(scene, counters=True)          # the counters build, a run of its own
        for S in [int(x) for x in args.samples.split(",")]:
            out = qc.hemisphere(pts, nrm, S, "cosine", seed=args.seed, skip=skip, fields=("open_count",))
            st = qc.stats()
            e = result["samples"][str(S)]
            total = n * S
            e["nodes_entered_per_sample"] = st["nodes_popped"] / total
            e["internal_nodes_per_sample"] = st["internal_visits"] / total
            e["triangle_tests_per_sample"] = st["triangle_tests"] / total
            e["open_fraction"] = st["misses"] / total
            assert int(out["open_count"].sum(dtype=torch.int64)) == st["misses"]
        qc.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
