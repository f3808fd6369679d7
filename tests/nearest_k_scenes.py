"""Scenes, points, radii and yardstick answers shared by test_nearest_k_host.py (CPU) and test_gpu_nearest_k.py -- TEST
INFRASTRUCTURE ONLY.  Everything is seeded and computed once per process.

* scene(name), sets(name): closest_point_scenes' scenes and point sets (N_SET points each; the first N_SET of teapot's
  uniform set).
* radii(name): {set: max_dist (N_SET,)}, one BOUNDED class per point in turn, built from the point's unbounded
  closest_point distance d (the host twin's; it only shapes the inputs) and the extent diagonal D:
    0, d, the float below d, the float above d, 1.5 d and 3 d (each capped at d + 1e-4 D, so that a point far away does
    not take in the whole mesh), 5e-5 D, 2e-4 D, negative.
  On teapot (a 6-unit mesh on a 2000-unit ground: D = 2828) 2e-4 D is 0.57 units, hundreds to thousands of triangles
  around a surface point; on the other scenes it is a small neighbourhood or nothing.
* unbounded(name): {set: (points, max_dist)}: the classes NaN, +inf, 1e19 in turn, all of which mean "everything"; the
  same points also run with max_dist = None.  N_UNBOUNDED points per set on the small scenes; on teapot, where every
  such query tests all 126,050 triangles, N_TEAPOT points of each of TEAPOT_GPU_SETS (64 in all) for the GPU tests, of
  which the yardstick takes the first N_TEAPOT_REF per set (16 in all).
* ref(name): the yardstick (nearest_k_ref.NearestKRef.walk) on the first N_REF points of every set with radii(), and
  on unbounded()'s points with the classes and with None.
"""
import functools

import numpy as np

import closest_point_scenes as CS
from closest_point_ref import F32, bound2
from nearest_k_ref import FIELDS, NearestKRef

SCENES = CS.SCENES
SMALL = tuple(s for s in SCENES if s != "teapot")
KS = (1, 2, 8, 64)
N_REF, N_SET = 300, 2000
N_TEAPOT, N_TEAPOT_REF = 16, 4      # per set of TEAPOT_GPU_SETS: every query there tests all 126,050 triangles
TEAPOT_GPU_SETS = ("uniform", "surface", "vertex", "non_finite")     # 4 x 16 = the 64 teapot points of the GPU tests
N_UNBOUNDED = 96         # per set on the small scenes
N_CLASSES = 9
scene = CS.scene


@functools.lru_cache(maxsize=None)
def sets(name):
    return {k: np.ascontiguousarray(v[:N_SET]) for k, v in CS.sets(name).items()}


@functools.lru_cache(maxsize=None)
def diagonal(name):
    return CS.extent(scene(name).arrays())[2]


def bounded_classes(d, D):
    d = np.ascontiguousarray(d, F32)
    cap = (d.astype(np.float64) + 1e-4 * D).astype(F32)
    out = np.zeros(d.shape[0], F32)
    with np.errstate(over="ignore"):
        for i in range(d.shape[0]):
            out[i] = (F32(0), d[i], np.nextafter(d[i], F32(0)), np.nextafter(d[i], F32(np.inf)),
                      min(d[i] * F32(1.5), cap[i]), min(d[i] * F32(3), cap[i]), F32(5e-5 * D), F32(2e-4 * D),
                      F32(-1.0))[i % N_CLASSES]
    return out


@functools.lru_cache(maxsize=None)
def radii(name):
    sc = scene(name)
    return {k: bounded_classes(sc.closest_point(p, fields=("distance",))["distance"], diagonal(name))
            for k, p in sets(name).items()}


@functools.lru_cache(maxsize=None)
def unbounded(name):
    cls = np.array([np.nan, np.inf, 1e19], F32)
    out = {}
    for k, p in sets(name).items():
        n = N_UNBOUNDED if name != "teapot" else N_TEAPOT if k in TEAPOT_GPU_SETS else 0
        out[k] = (np.ascontiguousarray(p[:n]), np.ascontiguousarray(cls[np.arange(n) % 3]))
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    return NearestKRef(scene(name))


@functools.lru_cache(maxsize=None)
def ref(name):
    """{set: dict(points, max_dist, walked: the bounded run on N_REF points; u_points, u_max_dist, u_walked, u_none:
    the unbounded runs with the classes and with None)}."""
    m = model(name)
    out = {}
    for k, pts in sets(name).items():
        p, md = np.ascontiguousarray(pts[:N_REF]), np.ascontiguousarray(radii(name)[k][:N_REF])
        nu = N_TEAPOT_REF if name == "teapot" else N_UNBOUNDED
        up, umd = (np.ascontiguousarray(x[:nu]) for x in unbounded(name)[k])
        assert all(bound2(x) == np.inf for x in umd[:3])     # the classes and None give one bound: one walk
        u = m.walk(up, umd)
        out[k] = dict(points=p, max_dist=md, walked=m.walk(p, md), u_points=up, u_max_dist=umd, u_walked=u, u_none=u)
    return out


@functools.lru_cache(maxsize=None)
def rows(name, set_name, run, k):
    """The yardstick's outputs for k of one run of ref(): run is "bounded", "classes" or "none"."""
    r = ref(name)[set_name]
    pts, walked = {"bounded": (r["points"], r["walked"]), "classes": (r["u_points"], r["u_walked"]),
                   "none": (r["u_points"], r["u_none"])}[run]
    return model(name).rows(pts, walked, k)


def differing_rows(got, want, fields=FIELDS):
    """Rows where a field of got differs from want's (bits, or NaN on both sides); dicts of arrays."""
    return CS.differing_rows(got, want, fields)
