"""Scenes, rays, bounds and yardstick answers shared by test_anyhit_order_ref.py (CPU) and
test_gpu_anyhit_order.py -- TEST INFRASTRUCTURE ONLY.  Everything is computed once per process.

* general(scene): the ray sets of test_gpu_trace_rays._ray_sets at 300 rays per set, with tmax = None and with
  test_gpu_query._tmax_classes over the oracle's closest t, answered by AnyHitOrderRef; general_ref(scene): the
  same rays and bounds answered by AnyHitRef.  teapot takes the four sets test_query_ref.py uses.
* deep(name, n): the constructed deep-chain sets of edge_scenes (axis_plus, solid_plus, tilted_plus and their
  interleaving) as prefixes of one N_DEEP-ray set each, so every size shares one pass of the model.

The Python yardsticks cost microseconds per traversal step; here the heaviest set (big_leaf, origins on
vertices) is 22,000 steps and the constructed deep sets 120 steps per ray, so no set is cut by a work budget:
every scene keeps all its rays.
"""
import atexit
import functools
import shutil
import tempfile

import numpy as np

import edge_scenes
import oracle_lib as O
import refit_ref as RR
from anyhit_ref import AnyHitOrderRef, AnyHitRef
from test_gpu_query import _tmax_classes
from test_gpu_trace_rays import _ray_sets

IMG = (16, 16, 1, 1)
SCENES = ["cornell", "cornell_plus", "spheres", "teapot", "cornell:no_bvh", "deep", "big_leaf", "same65"]
TEAPOT_SETS = ("random", "axis_aligned", "vertex_origin", "vertex_origin_zero_component")   # test_query_ref.SETS
N_REF = 300
N_DEEP = 4096
DEEP_SETS = ("axis_plus", "solid_plus", "tilted_plus")


@functools.lru_cache(maxsize=None)
def paths():
    d = tempfile.mkdtemp(prefix="anyhit_order_scenes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = dict(edge_scenes.write(d))
    out["same65"] = "%s/same65.scene" % d
    with open(out["same65"], "w") as f:
        f.write(RR.same_centroid_scene(65))
    return out


def scene_path(scene):
    """(path, use_bvh) of "name" or "name:no_bvh"."""
    name, _, flag = scene.partition(":")
    return paths().get(name) or "%s/%s.scene" % (O.ASSETS, name), flag != "no_bvh"


@functools.lru_cache(maxsize=None)
def oracle(scene):
    path, use_bvh = scene_path(scene)
    return O.OracleScene(path, use_bvh=use_bvh, image=IMG)


@functools.lru_cache(maxsize=None)
def model(scene):
    return AnyHitOrderRef(oracle(scene))


@functools.lru_cache(maxsize=None)
def plain(scene):
    return AnyHitRef(oracle(scene))


@functools.lru_cache(maxsize=None)
def general(scene):
    """{set: (rays, tm, {"none": (mask, ctr, depth, opops, opush), "classes": ...})}: the model's answers with
    tmax = None and with the bound classes tm."""
    orc, m = oracle(scene), model(scene)
    sets = _ray_sets(orc, np.random.default_rng(1234), N_REF)
    rng = np.random.default_rng(77)
    out = {}
    for k, rays in sets.items():
        if scene == "teapot" and k not in TEAPOT_SETS:
            continue
        r = np.ascontiguousarray(rays, np.float32)
        tm = _tmax_classes(orc.closest_hit(r)[0], rng)
        out[k] = (r, tm, {"none": m.batch(r, None), "classes": m.batch(r, tm)})
    return out


@functools.lru_cache(maxsize=None)
def general_ref(scene):
    """{set: {"none": (mask, ctr), "classes": (mask, ctr)}}: AnyHitRef on the rays and bounds of general(scene)."""
    p = plain(scene)
    return {k: {"none": p.batch(r, None), "classes": p.batch(r, tm)} for k, (r, tm, _) in general(scene).items()}


@functools.lru_cache(maxsize=None)
def _deep_full():
    orc, m = oracle("deep"), model("deep")
    rng = np.random.default_rng(78)
    out = {}
    for name in DEEP_SETS:
        r = getattr(edge_scenes, name)(N_DEEP)
        tm = _tmax_classes(orc.closest_hit(r)[0], rng)
        out[name] = (r, tm, {"none": m.batch(r, None), "classes": m.batch(r, tm)})
    return out


BIG_LEAF_SCENES = ["big_leaf", "same65", "same65:no_bvh"]
N_BIG = 256


def big_leaf_rays(n=N_BIG):
    """Rays at the fan of triangles around (0, 1, 0) that big_leaf and the same-centroid scenes keep in one leaf:
    test_gpu_edge_scenes.test_big_leaf_rays' set (from x = -4 toward +x), the same from the far side (x = +4
    toward -x), and rays from above and from below, which meet the fan and the ground quad in either order."""
    rng = np.random.default_rng(12)
    sides = []
    for sx in (-1.0, 1.0):
        o = np.hstack([np.full((n, 1), 4.0 * sx), rng.random((n, 2)) * [1.6, 1.6] + [0.2, -0.8]])
        d = np.hstack([np.full((n, 1), -sx), rng.normal(size=(n, 2)) * 0.05])
        sides.append(np.hstack([o, edge_scenes._unit(d)]))
    for sy in (-1.0, 1.0):
        xz = rng.random((n, 2)) * 1.6 - 0.8
        o = np.stack([xz[:, 0], np.full(n, 1.0 + 3.0 * sy), xz[:, 1]], 1)
        dn = rng.normal(size=(n, 2)) * 0.2
        d = np.stack([dn[:, 0], np.full(n, -sy), dn[:, 1]], 1)
        sides.append(np.hstack([o, edge_scenes._unit(d)]))
    # from the ground plane itself (y = 0 exactly) up into the fan: the quad's flat box is entered at distance 0,
    # before the fan's, and its triangles reject t = 0 < eps, so the big leaf is the far child that is popped
    xz = rng.random((n, 2)) * 4.0 - 2.0
    o = np.stack([xz[:, 0], np.zeros(n), xz[:, 1]], 1)
    aim = np.array([0.0, 1.0, 0.0]) + rng.normal(size=(n, 3)) * 0.2
    sides.append(np.hstack([o, edge_scenes._unit(aim - o)]))
    return np.ascontiguousarray(np.vstack(sides), np.float32)


@functools.lru_cache(maxsize=None)
def big_leaf(scene):
    """(rays, tm, {"none": (mask, ctr, ways), "classes": ...}) on big_leaf_rays(); ways counts how the model
    entered the leaf of more than 63 triangles: {"root": .., "selected": .., "popped": ..}."""
    orc, m = oracle(scene), model(scene)
    big = [i for i in range(len(m.child1)) if m.child1[i] - m.child2[i] > 63]
    assert len(big) == 1, big
    rays = big_leaf_rays()
    tm = _tmax_classes(orc.closest_hit(rays)[0], np.random.default_rng(79))
    res = {}
    for b, tmax in (("none", None), ("classes", tm)):
        mask, ctr = np.zeros(rays.shape[0], np.bool_), np.zeros((rays.shape[0], 4), np.int64)
        ways = {"root": 0, "selected": 0, "popped": 0}
        for i in range(rays.shape[0]):
            entered = []
            r = m.query(rays[i], None if tmax is None else tmax[i], entered)
            mask[i], ctr[i] = bool(r[0]), r[1:5]
            for node, how in entered:
                if node == big[0]:
                    ways[how] += 1
        res[b] = (mask, ctr, ways)
    return rays, tm, res


def _weave(parts, n):
    """Row i of each of the arrays (or lists) in turn, over their first n rows."""
    if isinstance(parts[0], list):
        return [p[i] for i in range(n) for p in parts]
    a = np.stack([p[:n] for p in parts], 1)
    return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))


@functools.lru_cache(maxsize=None)
def _deep_full_ref():
    p = plain("deep")
    return {k: {"none": p.batch(r, None), "classes": p.batch(r, tm)} for k, (r, tm, _) in _deep_full().items()}


def deep_ref(name, n):
    """{"none": (mask, ctr), "classes": ...}: AnyHitRef on the rays and bounds of deep(name, n)."""
    full = _deep_full_ref()
    if name != "interleaved":
        return {b: tuple(c[:n] for c in v) for b, v in full[name].items()}
    return {b: tuple(_weave([full[s][b][c] for s in DEEP_SETS], n) for c in range(2)) for b in ("none", "classes")}


def deep(name, n):
    """(rays, tm, {"none": (mask, ctr, depth, opops, opush), "classes": ...}) of the first n rays of a constructed
    set, or for name = "interleaved" of the 3 n rays that take ray i of each set in turn (with ray i's bound)."""
    full = _deep_full()
    assert n <= N_DEEP
    if name != "interleaved":
        r, tm, res = full[name]
        return (np.ascontiguousarray(r[:n]), np.ascontiguousarray(tm[:n]),
                {b: tuple(c[:n] for c in v) for b, v in res.items()})
    parts = [full[s] for s in DEEP_SETS]
    rays = edge_scenes.interleaved(*[p[0][:n] for p in parts])
    assert np.array_equal(rays, _weave([p[0] for p in parts], n))
    return (rays, _weave([p[1] for p in parts], n),
            {b: tuple(_weave([p[2][b][c] for p in parts], n) for c in range(5)) for b in ("none", "classes")})
