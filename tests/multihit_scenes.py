"""Scenes, rays, bounds and yardstick answers shared by test_multihit_host.py (CPU) and test_gpu_multihit.py -- TEST
INFRASTRUCTURE ONLY.  Everything is computed once per process.

* twins: four layers of two overlapping triangles, each triangle written twice with identical vertices, plus a sphere
  behind them.  A twin pair gives the same t bit for bit under two indices, so the order of the kept records is
  decided by the index; `through` rays cross all layers and then the sphere.
* ctx(scene): the product's and the oracle's scene at 16x16, test_gpu_trace_rays._ray_sets at 20,000 rays per set
  (plus `through` on twins and the deep-chain sets of edge_scenes on deep, where solid_plus crosses all 60
  triangles), the oracle's closest hits of the first N_REF rays and test_gpu_query._tmax_classes over them.
* ref(scene): MultiHitRef on the first N_REF rays of every set, with tmax = None and with the bound classes.
* deep(name, n): the first n rays of a constructed deep-chain set (or their interleaving) with MultiHitRef's answers.
"""
import atexit
import functools
import shutil
import tempfile

import numpy as np

import edge_scenes
import oracle_lib as O
import rtamd as R
from multihit_ref import MultiHitRef
from test_gpu_query import _tmax_classes
from test_gpu_trace_rays import _ray_sets

IMG = (16, 16, 1, 1)
SCENES = ["cornell", "cornell:no_bvh", "cornell_plus", "spheres", "teapot", "deep", "big_leaf", "twins"]
KS = (1, 2, 8, 64)
N_SETS, N_REF = 20000, 300
N_DEEP = 1024
DEEP_SETS = ("axis_plus", "solid_plus", "tilted_plus")
BOUNDS = ("none", "classes")
TWIN_LAYERS = 4


def twins_scene():
    s = edge_scenes.HEADER
    for layer in range(TWIN_LAYERS):
        z = -1.0 * layer
        for tri in (((-2.0, -2.0, z), (2.0, -2.0, z), (0.0, 2.0, z)),
                    ((-2.0, 2.0, z - 0.25), (2.0, 2.0, z - 0.25), (0.0, -2.0, z - 0.25))):
            s += edge_scenes._tri(*tri) * 2                       # the twin: the same line again
    s += "sphere grey 0 0 -8 1.5\n"
    s += "camera position 0 0 6 forward 0 0 -1 up 0 1 0 fov 40\n"
    s += "image 16 16 1 1 1\n"
    return s


def through(n, seed=31):
    """From z = 3 toward -z with a small tilt, inside both triangles of every layer: 16 triangle hits in 8 twin pairs,
    then (mostly) the sphere's near side."""
    rng = np.random.default_rng(seed)
    o = np.hstack([rng.random((n, 2)) * 0.6 - 0.3, np.full((n, 1), 3.0)])
    d = np.hstack([rng.normal(size=(n, 2)) * 0.02, np.full((n, 1), -1.0)])
    return np.ascontiguousarray(np.hstack([o, edge_scenes._unit(d)]), np.float32)


@functools.lru_cache(maxsize=None)
def paths():
    d = tempfile.mkdtemp(prefix="multihit_scenes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = dict(edge_scenes.write(d))
    out["twins"] = "%s/twins.scene" % d
    with open(out["twins"], "w") as f:
        f.write(twins_scene())
    return out


def scene_path(scene):
    """(path, use_bvh) of "name" or "name:no_bvh"."""
    name, _, flag = scene.partition(":")
    return paths().get(name) or "%s/%s.scene" % (O.ASSETS, name), flag != "no_bvh"


@functools.lru_cache(maxsize=None)
def ctx(scene):
    """dict(orc, dev, sets: {name: rays (20000 or fewer, 6)}, t_c: {name: oracle closest t of the first N_REF},
    i_c: the same for index, tm: {name: bound classes of the first N_REF})."""
    path, use_bvh = scene_path(scene)
    orc, dev = O.OracleScene(path, use_bvh=use_bvh, image=IMG), R.Scene(path, use_bvh=use_bvh, image=IMG)
    sets = _ray_sets(orc, np.random.default_rng(1234), N_SETS)
    if scene == "twins":
        sets["through"] = through(N_SETS)
    if scene == "deep":
        for name in DEEP_SETS:
            sets[name] = getattr(edge_scenes, name)(N_DEEP)
    sets = {k: np.ascontiguousarray(v, np.float32) for k, v in sets.items()}
    rng = np.random.default_rng(77)
    t_c, i_c, tm = {}, {}, {}
    for k, rays in sets.items():
        t_c[k], i_c[k] = orc.closest_hit(np.ascontiguousarray(rays[:N_REF]))[:2]
        tm[k] = _tmax_classes(t_c[k], rng)
    return dict(orc=orc, dev=dev, sets=sets, t_c=t_c, i_c=i_c, tm=tm)


@functools.lru_cache(maxsize=None)
def model(scene):
    return MultiHitRef(ctx(scene)["orc"])


@functools.lru_cache(maxsize=None)
def ref(scene):
    """{set: (rays (N_REF, 6), tm, {"none": (records, count, ctr, depth), "classes": ...})}."""
    c, m = ctx(scene), model(scene)
    out = {}
    for k, rays in c["sets"].items():
        r = np.ascontiguousarray(rays[:N_REF])
        out[k] = (r, c["tm"][k], {"none": m.batch(r, None), "classes": m.batch(r, c["tm"][k])})
    return out


@functools.lru_cache(maxsize=None)
def _deep_full():
    c, m = ctx("deep"), model("deep")
    rng = np.random.default_rng(78)
    out = {}
    for name in DEEP_SETS:
        r = c["sets"][name]
        tm = _tmax_classes(c["orc"].closest_hit(r)[0], rng)
        out[name] = (r, tm, {"none": m.batch(r, None), "classes": m.batch(r, tm)})
    return out


def _weave(parts, n):
    """Row i of each of the arrays (or lists) in turn, over their first n rows."""
    if isinstance(parts[0], list):
        return [p[i] for i in range(n) for p in parts]
    a = np.stack([p[:n] for p in parts], 1)
    return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))


def deep(name, n):
    """(rays, tm, {"none": (records, count, ctr, depth), "classes": ...}) of the first n rays of a constructed set, or
    for name = "interleaved" of the 3 n rays that take ray i of each set in turn (with ray i's bound)."""
    full = _deep_full()
    assert n <= N_DEEP
    if name != "interleaved":
        r, tm, res = full[name]
        return (np.ascontiguousarray(r[:n]), np.ascontiguousarray(tm[:n]), {b: tuple(c[:n] for c in v) for b, v in res.items()})
    parts = [full[s] for s in DEEP_SETS]
    rays = edge_scenes.interleaved(*[p[0][:n] for p in parts])
    return (rays, _weave([p[1] for p in parts], n),
            {b: tuple(_weave([p[2][b][c] for p in parts], n) for c in range(4)) for b in BOUNDS})
