"""Record what rt_trace_rays returns for 257 fixed rays on cornell (tests/test_gpu_trace_rays.py,
test_trace_rays_pinned): t, index and every rt_stats field, with the work counters on and off.  257 rays
fill one 256-thread workgroup and put one lane in the next.  The rays themselves are stored, so the pin
does not depend on a random generator's stream.

Run on a GPU with the library whose behaviour is to be pinned (RTAMD_LIB selects a build):
    python tests/golden/make_trace_rays_pin.py [out.npz]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "cuda-raytracer_amd"))
import rtamd as R  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "trace_rays_pin.npz")
N = 257


def rays():
    rng = np.random.default_rng(20260257)
    # origins around the camera side of the box (the box spans about [-1, 1] x [0, 2] x [-1, 1]), some outside it
    o = (np.array([0.0, 1.0, 1.5]) + rng.normal(size=(N, 3)) * np.array([0.8, 0.8, 1.2])).astype(np.float32)
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d[::16, rng.integers(0, 3)] = 0.0                    # an exactly zero component: 1/d = inf
    d = (d / np.sqrt((d * d).sum(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
    return np.ascontiguousarray(np.hstack([o, d]), np.float32)


def main():
    scene = R.Scene("%s/cornell.scene" % R.ASSETS, image=(16, 16, 1, 1))
    r = rays()
    out = {"rays": r}
    for name, on in (("on", True), ("off", False)):
        t, idx, st = R.trace_rays(scene, r, counters=on)
        out["t_" + name] = t.view(np.uint32)
        out["index_" + name] = idx
        out["stats_" + name] = np.array(json.dumps(st, sort_keys=True))
        print(name, "hits", int((idx >= 0).sum()), st)
    np.savez(OUT, **out)


if __name__ == "__main__":
    main()
