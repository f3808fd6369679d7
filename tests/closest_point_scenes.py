"""Scenes, points, bounds and yardstick answers shared by test_closest_point_host.py (CPU) and
test_gpu_closest_point.py -- TEST INFRASTRUCTURE ONLY.  Everything is seeded and computed once per process.

* scene(name): the product loader's scene (rtamd.Scene) of a shipped scene, an edge scene (deep, big_leaf) or twins
  (multihit_scenes: every triangle written twice, so a twin pair is equally near under two indices).
* sets(name): {set: points (N_SET, 3) float32} -- uniform in the bounds inflated by 25 % (N_BIG on teapot), on random
  triangles, 1e-3 along the normal off random triangles, 1000 diagonals away, exactly at vertices, non_finite
  (NaN / +inf / -inf components, finite rows in between), and over_twins on twins.
* bound_classes(distance): one max_dist class per point in turn: 0, the distance, the floats just below and above it,
  half of it, negative, NaN, +inf, 1e19.  (NULL is the run without max_dist.)
* ref(name): the yardstick (closest_point_ref.ClosestPointRef) on the first N_REF points of every set, without
  max_dist and with the bound classes.
"""
import functools

import numpy as np

import multihit_scenes as MS
import rtamd as R
from closest_point_ref import F32, ClosestPointRef

SCENES = MS.SCENES          # cornell, cornell:no_bvh, cornell_plus, spheres, teapot, deep, big_leaf, twins
N_REF, N_SET, N_BIG = 300, 2000, 20000
BOUNDS = ("none", "classes")
FIELDS = ("distance", "index", "point", "uv")
FINITE_SETS = ("uniform", "surface", "off_surface", "far", "vertex")


@functools.lru_cache(maxsize=None)
def scene(name):
    path, use_bvh = MS.scene_path(name)
    return R.Scene(path, use_bvh=use_bvh, image=MS.IMG)


def extent(arr):
    """(lo, hi, diagonal) of the triangles' root box and the spheres, float64."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    if arr["triangles"].shape[0]:
        lo, hi = arr["bvh"][0, 0:3].astype(np.float64), arr["bvh"][0, 3:6].astype(np.float64)
    for s in arr["spheres"].astype(np.float64):
        lo, hi = np.minimum(lo, s[0:3] - s[3]), np.maximum(hi, s[0:3] + s[3])
    return lo, hi, float(np.sqrt(((hi - lo) ** 2).sum()))


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _on_surface(arr, n, rng, off=0.0):
    """Points on random triangles (on random spheres in a scene without triangles), moved `off` along the normal."""
    T = arr["triangles"].astype(np.float64)
    if T.shape[0] == 0:
        s = arr["spheres"].astype(np.float64)[rng.integers(0, arr["spheres"].shape[0], n)]
        return s[:, 0:3] + (s[:, 3:4] + off) * _unit(rng.normal(size=(n, 3)))
    t = T[rng.integers(0, T.shape[0], n)]
    a, b = rng.random(n), rng.random(n)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    return t[:, 0:3] + a[:, None] * t[:, 3:6] + b[:, None] * t[:, 6:9] + off * np.nan_to_num(t[:, 9:12])


@functools.lru_cache(maxsize=None)
def sets(name):
    arr = scene(name).arrays()
    lo, hi, diag = extent(arr)
    rng = np.random.default_rng([4711, SCENES.index(name)])
    n_uni = N_BIG if name == "teapot" else N_SET
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.25
    out = {"uniform": mid + (rng.random((n_uni, 3)) * 2 - 1) * half,
           "surface": _on_surface(arr, N_SET, rng),
           "off_surface": _on_surface(arr, N_SET, rng, 1e-3),
           "far": mid + 1000.0 * diag * _unit(rng.normal(size=(N_SET, 3)))}
    T = arr["triangles"]
    if T.shape[0]:
        t = T[rng.integers(0, T.shape[0], N_SET)]
        corner = rng.integers(0, 3, N_SET)
        v = np.where((corner == 0)[:, None], t[:, 0:3], np.where((corner == 1)[:, None], t[:, 0:3] + t[:, 3:6],
                                                                 t[:, 0:3] + t[:, 6:9]))
        out["vertex"] = v.astype(F32)                       # float32 sums: the vertices the records give
    else:
        out["vertex"] = arr["spheres"][rng.integers(0, arr["spheres"].shape[0], N_SET), 0:3]   # the centres: len == 0
    nf = np.array(out["uniform"][:N_SET], np.float64)
    bad = (np.nan, np.inf, -np.inf)
    for i in range(N_SET):
        if i % 4 != 3:                                      # every fourth row stays finite
            nf[i, (i // 4) % 3] = bad[i % 4]
    out["non_finite"] = nf
    if name == "twins":
        out["over_twins"] = np.hstack([rng.random((N_SET, 2)) * 0.6 - 0.3, rng.random((N_SET, 1)) * 5 - 4])
    return {k: np.ascontiguousarray(v, F32) for k, v in out.items()}


def bound_classes(distance):
    """One class per point in turn, from the unbounded distance d: 0, d, the float below d, the float above d, d / 2,
    negative, NaN, +inf, 1e19."""
    d = np.ascontiguousarray(distance, F32)
    out = np.zeros(d.shape[0], F32)
    for i in range(d.shape[0]):
        out[i] = (F32(0), d[i], np.nextafter(d[i], F32(0)), np.nextafter(d[i], F32(np.inf)), d[i] * F32(0.5), F32(-1.0),
                  F32(np.nan), F32(np.inf), F32(1e19))[i % 9]
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    return ClosestPointRef(scene(name))


@functools.lru_cache(maxsize=None)
def ref(name):
    """{set: (points (N_REF, 3), max_dist (N_REF,), {"none": batch dict, "classes": batch dict})}."""
    m = model(name)
    out = {}
    for k, pts in sets(name).items():
        p = np.ascontiguousarray(pts[:N_REF])
        none = m.batch(p)
        md = bound_classes(none["distance"])
        out[k] = (p, md, {"none": none, "classes": m.batch(p, md)})
    return out


def differing_rows(got, want, fields=FIELDS):
    """Rows where a field of got differs from want's (bits, or NaN on both sides); dicts of arrays."""
    from closest_point_ref import same
    bad = np.zeros(np.asarray(want[fields[0]]).shape[0], bool) if fields else np.zeros(0, bool)
    for f in fields:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, g.dtype, w.shape, w.dtype)
        eq = same(g, w) if w.dtype == np.float32 else g == w
        bad |= ~eq.reshape(eq.shape[0], int(np.prod(eq.shape[1:]))).all(1)
    return np.nonzero(bad)[0]
