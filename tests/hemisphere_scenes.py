"""Scenes, frames, filters and yardstick answers shared by test_hemisphere_host.py (CPU) and test_gpu_hemisphere.py -- TEST
INFRASTRUCTURE ONLY.  Everything is computed once per process.

* scenes and ray sets are multihit_scenes' (tests/multihit_scenes.py), by import.
* frames(scene, set): one frame per ray of the set's first N_REF rays.  Points and normals are Scene.hit_records
  (position, normal turned against the ray) of the oracle's closest hits (t_c, i_c); skip = i_c.  Classes, cycled over
  the rows (row i has class i mod 8; 0, 1, 2 leave the hit frame as it is):
    3  the normal scaled to length 3;          4  a zero normal;          5  a NaN normal;
    6  a miss: point = the ray's origin, normal = -d (every row the oracle missed is of this class too);
    7  a point far outside the scene (the hit point + 1e6 along x), the normal kept.
* filters(scene, set): the runs "own" (skip = i_c, nothing else) and ray_filter_scenes' "tmax", "skip", "mask" and "all",
  one row per frame.
* ref(scene): HemisphereRef over the first 300 work items (16 on teapot) of every set and run, rounded down to whole
  points: S = 3 in cosine mode (100 points; 5 on teapot), and for the runs "own" and "all" also S = 64 in uniform mode
  (4 points; S = 16 and 1 point on teapot).
* deep_frames(): point = origin and normal = direction of the first DEEP_FRAMES rays of each of deep's constructed
  sets, with the depth the yardstick walk reaches over S = 4096 samples each.  FINDING: no sample goes
  deeper than DEEP_DEPTH = 1 entry.  The chain pushes one entry per level only for a ray that stays inside the
  triangles' common yz box (|y|, |z| <= 1.2) out to x = 3^k, k > 46 for more than 16 entries, i.e. within 1e-22 rad of
  +x; a sample direction is normalise(n + u) with u's tangential part a multiple of about 2^-15.5 or exactly 0, and 0
  needs u = +-n exactly, which random_on_sphere gives only for n = (0, 0, +-1).  The rays themselves (the sets' own
  directions) reach 26 to 29 entries, which tests/test_gpu_ray_filter.py walks through the same loop text.
"""
import functools

import numpy as np

import multihit_scenes as M
import ray_filter_scenes as FS
from hemisphere_ref import HemisphereRef

SCENES = M.SCENES
RUNS = ("own", "tmax", "skip", "mask", "all")
MEMBERS = FS.MEMBERS
N_REF = M.N_REF
MODES = (("cosine", 3), ("uniform", 64))     # (mode, S) of the yardstick runs
MODES_TEAPOT = (("cosine", 3), ("uniform", 16))
DEEP_FRAMES = 2
DEEP_SAMPLES = 4096
DEEP_DEPTH = 1
ANYHIT_LDS = 16


def modes_of(run, scene=None):
    m = MODES_TEAPOT if scene == "teapot" else MODES
    return m if run in ("own", "all") else m[:1]


def n_items(scene):
    return 16 if scene == "teapot" else 300


@functools.lru_cache(maxsize=None)
def frames(scene, name):
    """(points (N_REF, 3), normals (N_REF, 3), skip (N_REF,) int32) of the set's first N_REF rays."""
    c = M.ctx(scene)
    rays = np.ascontiguousarray(c["sets"][name][:N_REF])
    t_c, i_c = c["t_c"][name], c["i_c"][name]
    rec = c["dev"].hit_records(rays, np.ascontiguousarray(t_c, np.float32), np.ascontiguousarray(i_c, np.int32),
                               ("normal", "position"))
    d = rays[:, 3:6]
    with np.errstate(all="ignore"):
        away = (rec["normal"] * d).sum(1) > 0
    nrm = np.where(away[:, None], -rec["normal"], rec["normal"]).astype(np.float32)
    pts = rec["position"].astype(np.float32).copy()
    k = np.arange(rays.shape[0]) % 8
    with np.errstate(all="ignore"):
        ln = np.sqrt((nrm * nrm).sum(1, keepdims=True)).astype(np.float32)
        nrm = np.where((k == 3)[:, None], np.float32(3) * nrm / np.where(ln > 0, ln, 1), nrm).astype(np.float32)
    nrm[k == 4] = 0
    nrm[k == 5] = np.nan
    miss = (k == 6) | (i_c < 0)
    pts[miss], nrm[miss] = rays[miss, :3], -rays[miss, 3:6]
    pts[k == 7, 0] += np.float32(1e6)
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm), np.ascontiguousarray(i_c, np.int32)


@functools.lru_cache(maxsize=None)
def filters(scene, name):
    """{run: dict(tmin, tmax, skip, mask, masks)}, one row per frame."""
    own = frames(scene, name)[2]
    n = own.shape[0]
    base = FS.filters(scene, name, n)
    out = {"own": dict(tmin=None, tmax=None, skip=own, mask=None, masks=None)}
    for run in ("tmax", "skip", "mask", "all"):
        out[run] = dict(base[run])
    return out


def members(f, n=None):
    return {k: (None if f[k] is None else np.ascontiguousarray(f[k][:n])) for k in MEMBERS}


def tiled(a, n):
    """Rows repeated to n."""
    return None if a is None else np.ascontiguousarray(np.resize(a, (n,) + a.shape[1:]))


@functools.lru_cache(maxsize=None)
def model(scene, masked):
    return HemisphereRef(M.ctx(scene)["dev"].arrays(), FS.prim_masks(scene) if masked else None)


@functools.lru_cache(maxsize=None)
def ref(scene):
    """{set: {run: {mode: (points, normals, members, masks, S, HemisphereRef.run's dict)}}}: the frames are the first
    n_items // S of the set, every sample of each walked."""
    out = {}
    items = n_items(scene)
    for name in M.ctx(scene)["sets"]:
        pts, nrm, _ = frames(scene, name)
        out[name] = {}
        for run, f in filters(scene, name).items():
            out[name][run] = {}
            for mode, S in modes_of(run, scene):
                n = items // S
                fm = members(f, n)
                res = model(scene, f["masks"] is not None).run(pts[:n], nrm[:n], S, mode, seed=11, **fm)
                out[name][run][mode] = (pts[:n], nrm[:n], fm, f["masks"], S, res)
    return out


@functools.lru_cache(maxsize=None)
def deep_frames():
    """(points, normals, deepest stack of the yardstick walk over DEEP_SAMPLES cosine samples per frame)."""
    c = M.ctx("deep")
    r = np.concatenate([c["sets"][name][:DEEP_FRAMES] for name in M.DEEP_SETS])
    pts, nrm = np.ascontiguousarray(r[:, :3]), np.ascontiguousarray(r[:, 3:6])
    res = model("deep", False).run(pts, nrm, DEEP_SAMPLES, "cosine", seed=3)
    return pts, nrm, res["depth"], res["open_count"]
