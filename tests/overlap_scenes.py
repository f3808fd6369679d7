"""Scenes, boxes and yardstick answers shared by test_overlap_host.py (CPU) and test_gpu_overlap.py -- TEST
INFRASTRUCTURE ONLY.  Everything is seeded and computed once per process.

* scene(name): closest_point_scenes' scenes (the shipped ones, deep, big_leaf, twins).  D is the extent diagonal.
* sets(name): {set: boxes (n, 6) float32 {lo.xyz, hi.xyz}}, N_SET boxes each (N_TEAPOT on teapot):
    uniform   centre uniform in the extent inflated by 25 %, half-extents log-uniform in [1e-4 D, 0.2 D] per axis;
    surface   centred on points of random triangles (spheres in a scene without triangles), half-extents log-uniform
              in [1e-5 D, 1e-3 D] per axis -- on teapot (D = 2828) 0.03 to 2.8 units around a 6-unit mesh;
    graze     one face placed exactly on a coordinate of a triangle's vertex (the float32 vertex the record gives), on
              the float just below it and on the float just above it, in turn; the box spans the vertex on the other axes;
    thin      one, two or three zero half-extents in turn (a rectangle, a segment, a point), half on surface points;
    inside    (teapot, spheres) cubes strictly inside the teapot's body, closer to their centre than the nearest
              surface, and cubes inside the first sphere of `spheres`;
    all       the whole extent, the extent inflated by 25 % and its lower half;
    invalid   uniform's boxes with three of every four made invalid: a NaN, +inf, -inf or lo > hi on one axis.
  No coordinate of uniform or surface is taken from a vertex.
* ref(name): the yardstick (overlap_ref.OverlapRef.walk) on the first N_REF boxes of every set.
"""
import functools

import numpy as np

import closest_point_scenes as CS
from closest_point_ref import F32
from overlap_ref import FIELDS, OverlapRef

SCENES = CS.SCENES
SMALL = tuple(s for s in SCENES if s != "teapot")
KS = (1, 2, 8, 64)
N_REF, N_SET, N_TEAPOT = 300, 2000, 256
scene = CS.scene


@functools.lru_cache(maxsize=None)
def extent(name):
    return CS.extent(scene(name).arrays())


def diagonal(name):
    return extent(name)[2]


def _log_uniform(rng, shape, a, b):
    return np.exp(rng.uniform(np.log(a), np.log(b), shape))


def _box(centre, half):
    c, h = np.asarray(centre, np.float64), np.asarray(half, np.float64)
    lo, hi = (c - h).astype(F32), (c + h).astype(F32)
    return np.ascontiguousarray(np.hstack([np.minimum(lo, hi), np.maximum(lo, hi)]), F32)


def _vertices32(arr, rng, n):
    """n random vertices as the records give them in float32 (p1, p1 + e1, p1 + e2); sphere centres without triangles."""
    T = arr["triangles"]
    if T.shape[0] == 0:
        return np.ascontiguousarray(arr["spheres"][rng.integers(0, arr["spheres"].shape[0], n), 0:3], F32)
    t = T[rng.integers(0, T.shape[0], n)].astype(F32)
    corner = rng.integers(0, 3, n)
    return np.where((corner == 0)[:, None], t[:, 0:3], np.where((corner == 1)[:, None], t[:, 0:3] + t[:, 3:6],
                                                                t[:, 0:3] + t[:, 6:9])).astype(F32)


def _graze(arr, rng, n, D):
    v = _vertices32(arr, rng, n)
    half = _log_uniform(rng, (n, 3), 1e-4 * D, 1e-2 * D)
    b = _box(v, half)
    axis, high = rng.integers(0, 3, n), rng.integers(0, 2, n).astype(bool)
    for i in range(n):
        c = int(axis[i])
        x = v[i, c]
        face = (x, np.nextafter(x, F32(-np.inf)), np.nextafter(x, F32(np.inf)))[i % 3]
        if high[i]:                                          # the box ends at the vertex coordinate
            b[i, 3 + c] = face
            b[i, c] = min(F32(np.float64(face) - 2 * half[i, c]), face)
        else:                                               # the box starts there
            b[i, c] = face
            b[i, 3 + c] = max(F32(np.float64(face) + 2 * half[i, c]), face)
    return b


def _inside(name, arr, rng, n):
    if name == "spheres":
        c, r = arr["spheres"][0, 0:3].astype(np.float64), float(arr["spheres"][0, 3])
        centre = c + (rng.random((n, 3)) * 2 - 1) * (r / 6)
        return _box(centre, np.full((n, 3), r / 6))          # farthest corner at most r sqrt(3) / 3 from c
    sc = scene(name)
    T = arr["triangles"].astype(np.float64)
    mesh = T[np.sqrt((T[:, 3:6] ** 2).sum(1)) < 10][:, 0:3]   # without the ground's two triangles
    lo, hi = mesh.min(0), mesh.max(0)
    out = np.zeros((0, 6), F32)
    while out.shape[0] < n:
        p = np.ascontiguousarray(lo + (hi - lo) * rng.random((8 * n, 3)), F32)
        d = sc.closest_point(p, fields=("distance",))["distance"]
        keep = (sc.signed_distance(p) < 0) & (d > 0.02)
        # a cube whose half-diagonal is half the distance to the nearest surface
        out = np.vstack([out, _box(p[keep], np.repeat(d[keep, None].astype(np.float64) / (2 * np.sqrt(3)), 3, 1))])
    return np.ascontiguousarray(out[:n])


@functools.lru_cache(maxsize=None)
def sets(name):
    arr = scene(name).arrays()
    lo, hi, D = extent(name)
    rng = np.random.default_rng([1913, SCENES.index(name)])
    n = N_TEAPOT if name == "teapot" else N_SET
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.25
    out = {"uniform": _box(mid + (rng.random((n, 3)) * 2 - 1) * half, _log_uniform(rng, (n, 3), 1e-4 * D, 0.2 * D)),
           "surface": _box(CS._on_surface(arr, n, rng), _log_uniform(rng, (n, 3), 1e-5 * D, 1e-3 * D)),
           "graze": _graze(arr, rng, n, D)}
    centre = np.vstack([CS._on_surface(arr, n // 2, rng), mid + (rng.random((n - n // 2, 3)) * 2 - 1) * half])
    h = _log_uniform(rng, (n, 3), 1e-4 * D, 0.05 * D)
    for i in range(n):
        zero = rng.permutation(3)[:1 + i % 3]
        h[i, zero] = 0.0
    out["thin"] = _box(centre, h)
    if name in ("teapot", "spheres"):
        out["inside"] = _inside(name, arr, rng, min(n, 256))
    out["all"] = np.vstack([_box(mid, (hi - lo) / 2), _box(mid, half), _box(mid - (hi - lo) / 4, (hi - lo) / 4)])
    bad = out["uniform"].copy()
    for i in range(n):
        c = (i // 4) % 3
        if i % 4 == 0:
            bad[i, (c, 3 + c)[(i // 12) % 2]] = np.nan
        elif i % 4 == 1:
            bad[i, (3 + c, c)[(i // 12) % 2]] = (np.inf, -np.inf)[(i // 12) % 2]
        elif i % 4 == 2:                                    # lo > hi on one axis, both finite
            bad[i, c], bad[i, 3 + c] = np.nextafter(bad[i, 3 + c], F32(np.inf)), bad[i, c]
    out["invalid"] = bad                                    # every fourth row stays valid
    return {k: np.ascontiguousarray(v, F32) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def model(name):
    return OverlapRef(scene(name))


@functools.lru_cache(maxsize=None)
def ref(name):
    """{set: dict(boxes (<= N_REF, 6), walked: OverlapRef.walk's results)}."""
    m = model(name)
    out = {}
    for k, b in sets(name).items():
        b = np.ascontiguousarray(b[:N_REF])
        out[k] = dict(boxes=b, walked=m.walk(b))
    return out


@functools.lru_cache(maxsize=None)
def rows(name, set_name, k):
    """The yardstick's outputs for k of one set of ref()."""
    return model(name).rows(ref(name)[set_name]["walked"], k)


def differing_rows(got, want, fields=FIELDS):
    """Rows where a field of got differs from want's; dicts of integer arrays."""
    return CS.differing_rows(got, want, fields)
