#!/usr/bin/env python3
"""Time from a mesh in arrays to a built scene (rtamd.Scene.from_mesh), outside bench.py.

Two meshes: teapot's triangles (Scene(teapot).vertices(), fed back as a soup with the file's materials) and the
40,961-triangle soup of tests/bvh_build_cases.py (size_40961).  After `--warmup` rounds, `--calls` timed rounds with
one call of every leg per round in a seeded shuffled order; every call is synchronous, so the time is host wall-clock
around the call; medians are reported.  Legs, per mesh:

  a_file_device   what a caller did before: rt_scene_load of a triangle-line file written beforehand, bvh_device=0
                  (write_file_ms, the writing of that file, is timed once, apart)
  b_host          from_mesh, numpy arrays, host build
  c_host_arrays_device_build   from_mesh, numpy arrays, bvh_device=0 (the host pre-pass, upload, level loop, download)
  d_device_tensors             from_mesh, torch tensors on cuda:0 (assemble kernel, level loop, finalize kernel)

After the timed rounds one (c) and one (d) build run in child processes (three untimed builds first) with
RTAMD_TIMING set; the builders' phase lines are kept.  Prints one JSON line and writes it to
profiles/mesh/mesh_bench.json (or --out).

    python tools/mesh_bench.py [--calls 10] [--warmup 3] [--seed 1] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import torch   # before the library loads, so that both run on one HIP runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cuda-raytracer_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import numpy as np   # noqa: E402
import rtamd   # noqa: E402

IMAGE = (16, 16, 1, 1)


def meshes():
    import bvh_build_cases
    import make_envmap
    make_envmap.ensure_envmap(os.path.join(REPO, "assets", "teapot", "textures", "envmap.pfm"))
    src = rtamd.Scene(os.path.join(rtamd.ASSETS, "teapot.scene"), image=IMAGE)
    a = src.arrays()
    yield "teapot", src.vertices(), a["materials"], a["material_indices"]
    import mesh_cases
    yield "size_40961", bvh_build_cases.vertices("size_40961"), mesh_cases.MATERIALS, bvh_build_cases.materials("size_40961")


def write_file(path, soup, materials, face_materials):
    """The parent commit's only route: one `triangle` text line per face."""
    import mesh_cases
    with open(path, "w") as f:
        f.write(mesh_cases.canonical_text(dict(vertices=soup, materials=materials, face_materials=face_materials)))


def timing_child(kind, npz):
    code = ("import sys, torch, numpy as np\nsys.path[:0] = %r\nimport rtamd\nz = np.load(%r)\n"
            "v, m, fm = z['v'], z['m'], z['fm']\n" % ([os.path.join(REPO, "cuda-raytracer_amd")], npz))
    if kind == "c":
        code += "for _ in range(3): rtamd.Scene.from_mesh(v, None, m, fm, image=%r, bvh_device=0)\n" % (IMAGE,)
        code += "import os; os.environ['RTAMD_TIMING'] = '1'\nrtamd.Scene.from_mesh(v, None, m, fm, image=%r, bvh_device=0)\n" % (IMAGE,)
    else:
        code += "tv, tfm = torch.from_numpy(v).cuda(), torch.from_numpy(fm).cuda()\n"
        code += "for _ in range(3): rtamd.Scene.from_mesh(tv, None, m, tfm, image=%r)\n" % (IMAGE,)
        code += "import os; os.environ['RTAMD_TIMING'] = '1'\nrtamd.Scene.from_mesh(tv, None, m, tfm, image=%r)\n" % (IMAGE,)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("timing child failed: " + r.stderr[-2000:])
    return [ln.strip() for ln in r.stderr.splitlines() if ln.startswith("gpu_build_")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh", "mesh_bench.json"))
    args = ap.parse_args()
    if args.calls < 1:
        ap.error("--calls must be at least 1")
    if not torch.cuda.is_available() or rtamd.device_count() < 1:
        sys.exit("mesh_bench: no HIP device")
    torch.cuda.set_device(0)
    rtamd.warmup(0)
    rng = random.Random(args.seed)
    result = {"calls": args.calls, "warmup": args.warmup, "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "clock": "host wall-clock around each synchronous call, ms", "meshes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, soup, materials, face_materials in meshes():
            soup = np.ascontiguousarray(soup, np.float32)
            face_materials = np.ascontiguousarray(face_materials, np.uint16)
            path = os.path.join(tmp, name + ".scene")
            t0 = time.perf_counter()
            write_file(path, soup, materials, face_materials)
            write_ms = (time.perf_counter() - t0) * 1e3
            tv, tfm = torch.from_numpy(soup).cuda(), torch.from_numpy(face_materials).cuda()
            torch.cuda.synchronize()
            legs = {
                "a_file_device": lambda: rtamd.Scene(path, image=IMAGE, bvh_device=0),
                "b_host": lambda: rtamd.Scene.from_mesh(soup, None, materials, face_materials, image=IMAGE),
                "c_host_arrays_device_build": lambda: rtamd.Scene.from_mesh(soup, None, materials, face_materials,
                                                                            image=IMAGE, bvh_device=0),
                "d_device_tensors": lambda: rtamd.Scene.from_mesh(tv, None, materials, tfm, image=IMAGE),
            }
            ref = legs["b_host"]().arrays()
            for k, leg in legs.items():                 # the legs build one scene
                got = leg().arrays()
                assert all(got[f].tobytes() == ref[f].tobytes() for f in ("bvh", "triangles", "material_indices")), k
            times = {k: [] for k in legs}
            order = list(legs)
            for rnd in range(args.warmup + args.calls):
                rng.shuffle(order)
                for k in order:
                    t0 = time.perf_counter()
                    s = legs[k]()
                    dt = (time.perf_counter() - t0) * 1e3
                    del s
                    if rnd >= args.warmup:
                        times[k].append(dt)
            npz = os.path.join(tmp, name + ".npz")
            np.savez(npz, v=soup, m=np.ascontiguousarray(materials, np.float32), fm=face_materials)
            result["meshes"][name] = {
                "triangles": int(soup.shape[0]), "file_bytes": os.path.getsize(path), "write_file_ms": round(write_ms, 3),
                "median_ms": {k: round(statistics.median(v), 3) for k, v in times.items()},
                "min_ms": {k: round(min(v), 3) for k, v in times.items()},
                "max_ms": {k: round(max(v), 3) for k, v in times.items()},
                "timing_c": timing_child("c", npz), "timing_d": timing_child("d", npz),
            }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
