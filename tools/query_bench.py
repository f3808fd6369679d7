#!/usr/bin/env python3
"""Ray-query throughput on one GPU (rtamd.RayQuery / rt_query_*), outside bench.py.

Workload: teapot.scene at 1920x1080.  One batch of pixel-centre primary rays is generated in torch on the
device; the hemisphere batch starts at the primary rays' triangle hit points, cosine-distributed about the
triangle normal (turned towards the incoming ray), drawn from a seeded torch generator.  Timed, after a
warm-up, `--calls` times each in alternation (one call of every leg per round, the order within a round shuffled from the seed):

  closest_device    RayQuery.closest on the device tensors (resident scene, caller's stream)
  trace_rays_host   the one-shot rt_trace_rays on the same rays through host memory (a query object created,
                    scene uploaded, scratch allocated and freed, results copied back: per call)
  occluded_tmax     RayQuery.occluded on the hemisphere rays, tmax = 10 % of the scene diagonal
  occluded_any      the same rays, tmax = None
  closest_hemi      RayQuery.closest on the hemisphere rays (the closest-hit cost of the same rays)

and, on both ray sets (the hemisphere legs carry the suffix _hemi), the hit records of DESIGN §13:

  closest_hit_all         RayQuery.closest_hit with every field
  closest_hit_tiuv        the same with t, index and uv only
  closest_torch_records   a caller's alternative: RayQuery.closest, then the same fields in torch ops over
                          Scene.arrays() tensors (torch_records)

with the added time of each over the closest leg of the same rays and rounds (hit_added_ms).

Device calls are timed with HIP events on the calling stream (ms, median and min) and on the host's wall
clock around call + synchronise; the host call on the wall clock only.  Prints one JSON line and writes it to
profiles/query/query_bench.json (or --out).

    python tools/query_bench.py [--calls 20] [--warmup 3] [--seed 1] [--scene teapot] [--out FILE]
"""
import argparse
import json
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


def vec(v, dev):
    return torch.tensor([v.x, v.y, v.z], dtype=torch.float32, device=dev)


def unit(v):
    return v / v.norm(dim=1, keepdim=True)


def primary_rays(scene, dev):
    """Pixel-centre rays of the scene's camera (scene.cu:78-105 without the jitter), (W*H, 6)."""
    v = scene.view
    W, H = v.width, v.height
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                          torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    xc = ((x + 0.5) * v.inv_width).reshape(-1, 1)
    yc = ((y + 0.5) * v.inv_height).reshape(-1, 1)
    d = unit(vec(v.near_plane_top_left, dev) + xc * vec(v.scaled_right, dev) - yc * vec(v.scaled_up, dev))
    o = vec(v.camera_position, dev).expand_as(d)
    return torch.cat([o, d], dim=1).contiguous()


def hemisphere_rays(rays, t, index, tris, sphere_count, gen):
    """From the triangle hits of `rays`: origin = the hit point, direction cosine-distributed about the
    triangle's normal turned against the incoming ray."""
    keep = index >= sphere_count
    r, tt, tri = rays[keep], t[keep].unsqueeze(1), (index[keep] - sphere_count).long()
    o, d = r[:, :3], r[:, 3:]
    p = o + tt * d
    n = tris[tri, 9:12]
    n = torch.where((n * d).sum(1, keepdim=True) > 0, -n, n)
    u = torch.rand((p.shape[0], 2), generator=gen, device=p.device, dtype=torch.float32)
    rad, phi = u[:, :1].sqrt(), 2 * torch.pi * u[:, 1:]
    helper = torch.where(n[:, :1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device=p.device),
                         torch.tensor([0.0, 1.0, 0.0], device=p.device))
    bx = unit(torch.linalg.cross(n, helper))
    by = torch.linalg.cross(n, bx)
    w = unit(rad * phi.cos() * bx + rad * phi.sin() * by + (1 - u[:, :1]).clamp_min(0).sqrt() * n)
    return torch.cat([p, w], dim=1).contiguous()


def torch_records(q, rays, tris, spheres, mat_idx):
    """A caller's alternative to RayQuery.closest_hit: closest, then the hit-record fields in torch ops
    over Scene.arrays() tensors -- the gathers and the arithmetic, not the library's rounding."""
    t, index = q.closest(rays)
    S = spheres.shape[0]
    hit, is_tri = index >= 0, index >= S
    o, d = rays[:, :3], rays[:, 3:]
    pos = o + t.unsqueeze(1) * d
    if tris.shape[0]:
        rec = tris[(index - S).clamp_min(0).long()]
        p1, e1, e2, normal = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12]
        h = torch.linalg.cross(d, e2)
        f = 1 / (h * e1).sum(1)
        s = o - p1
        uv = torch.stack([(s * h).sum(1) * f, (d * torch.linalg.cross(s, e1)).sum(1) * f], 1)
        uv = torch.where(is_tri.unsqueeze(1), uv, torch.zeros_like(uv))
    else:
        uv, normal = torch.zeros((rays.shape[0], 2), device=rays.device), torch.zeros_like(pos)
    if S:
        sp = spheres[index.clamp(0, S - 1).long()]
        normal = torch.where(is_tri.unsqueeze(1), normal, (pos - sp[:, :3]) / sp[:, 3:4])
    zero = torch.zeros_like(pos)
    normal = torch.where(hit.unsqueeze(1), normal, zero)
    return {"t": t, "index": index, "uv": uv, "normal": normal, "position": torch.where(hit.unsqueeze(1), pos, zero),
            "material": torch.where(hit, mat_idx[index.clamp_min(0).long()], torch.full_like(index, -1)),
            "front_face": hit & ((normal * d).sum(1) < 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", default="teapot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "query", "query_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("query_bench: no HIP device")
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
    n = rays.shape[0]
    q.reserve(n)
    t, index = q.closest(rays)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    hemi = hemisphere_rays(rays, t, index, torch.from_numpy(arr["triangles"]).to(dev), scene.view.sphere_count, gen)
    nh = hemi.shape[0]
    tmax = torch.full((nh,), 0.1 * diag, dtype=torch.float32, device=dev)
    rays_host = rays.cpu().numpy()
    torch.cuda.synchronize()

    def device_call(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3, out
        return run

    def host_call():
        w0 = time.perf_counter()
        out = rtamd.trace_rays(scene, rays_host)
        return None, (time.perf_counter() - w0) * 1e3, out

    legs = [("closest_device", n, device_call(lambda: q.closest(rays))),
            ("trace_rays_host", n, host_call),
            ("occluded_tmax", nh, device_call(lambda: q.occluded(hemi, tmax))),
            ("occluded_any", nh, device_call(lambda: q.occluded(hemi))),
            ("closest_hemi", nh, device_call(lambda: q.closest(hemi)))]
    # hit records, when the library has them (the symbol is the feature probe: an A/B run on an
    # older library times the legs above alone)
    has_hit = hasattr(rtamd.lib(), "rt_query_closest_hit")
    if has_hit:
        tris_t, sph_t = torch.from_numpy(arr["triangles"]).to(dev), torch.from_numpy(arr["spheres"]).to(dev)
        mat_t = torch.from_numpy(arr["material_indices"].astype(np.int32)).to(dev)
        for tag, r, count in (("", rays, n), ("_hemi", hemi, nh)):
            legs += [("closest_hit_all" + tag, count, device_call(lambda r=r: q.closest_hit(r))),
                     ("closest_hit_tiuv" + tag, count, device_call(lambda r=r: q.closest_hit(r, fields=("t", "index", "uv")))),
                     ("closest_torch_records" + tag, count, device_call(lambda r=r: torch_records(q, r, tris_t, sph_t, mat_t)))]
    times = {name: ([], []) for name, _, _ in legs}
    shuffler = random.Random(args.seed)
    last = {}
    for k in range(args.warmup + args.calls):
        order = list(legs)                      # alternating: every leg once per round, in a seeded random order,
        shuffler.shuffle(order)                 # so that no leg always runs right after the same one
        for name, _, run in order:
            ev, wall, out = run()
            last[name] = out
            if k >= args.warmup:
                if ev is not None:
                    times[name][0].append(ev)
                times[name][1].append(wall)
    result = {"tool": "tools/query_bench.py", "scene": args.scene, "width": args.width, "height": args.height,
              "calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "scene_diagonal": diag, "tmax": 0.1 * diag, "legs": {}}
    for name, count, _ in legs:
        ev, wall = times[name]
        leg = {"rays": count, "wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall)}
        leg["mrays_per_s_wall"] = count / leg["wall_ms_median"] / 1e3
        if ev:
            leg.update(event_ms_median=statistics.median(ev), event_ms_min=min(ev))
            leg["mrays_per_s_event"] = count / leg["event_ms_median"] / 1e3
        result["legs"][name] = leg
    # what the timed calls computed: the resident and the one-shot closest hit agree bit for bit
    t_d, i_d = last["closest_device"]
    t_h, i_h, _ = last["trace_rays_host"]
    result["closest_matches_trace_rays"] = bool(
        np.array_equal(t_d.cpu().numpy().view(np.uint32), t_h.view(np.uint32)) and np.array_equal(i_d.cpu().numpy(), i_h))
    result["primary_hit_fraction"] = float((index >= 0).float().mean())
    result["occluded_tmax_fraction"] = float(last["occluded_tmax"].float().mean())
    result["occluded_any_fraction"] = float(last["occluded_any"].float().mean())
    result["occluded_any_equals_closest_hit"] = bool(torch.equal(last["occluded_any"], last["closest_hemi"][1] >= 0))
    result["speedup_closest_device_over_trace_rays_host_wall"] = (
        result["legs"]["trace_rays_host"]["wall_ms_median"] / result["legs"]["closest_device"]["wall_ms_median"])
    if has_hit:
        # the added time of closest_hit over closest in the same rounds, and against the torch alternative's
        for tag, base in (("", "closest_device"), ("_hemi", "closest_hemi")):
            ms = {k: result["legs"][k + tag]["event_ms_median"] for k in ("closest_hit_all", "closest_hit_tiuv", "closest_torch_records")}
            b = result["legs"][base]["event_ms_median"]
            result["hit_added_ms" + tag] = {k: v - b for k, v in ms.items()}
            result["hit_added_ratio_torch_over_closest_hit_all" + tag] = (
                (ms["closest_torch_records"] - b) / (ms["closest_hit_all"] - b) if ms["closest_hit_all"] > b else None)
            result["hit_ratio_torch_over_closest_hit_all" + tag] = ms["closest_torch_records"] / ms["closest_hit_all"]
            got, alt = last["closest_hit_all" + tag], last["closest_torch_records" + tag]
            fin = torch.isfinite(got["uv"]).all(1) & torch.isfinite(alt["uv"]).all(1)
            result["torch_records_max_abs_diff" + tag] = {
                k: float((got[k][fin] - alt[k][fin]).abs().max()) for k in ("uv", "normal", "position")}
            result["torch_records_material_equal" + tag] = bool(torch.equal(got["material"], alt["material"]))
    q.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
