"""Yardsticks for the refit (rt_scene_refit, rt_query_update_triangles) -- TEST INFRASTRUCTURE ONLY.

* refit_numpy(bvh, vertices): the definition of include/rt_abi.h restated.  Triangle records in float32 numpy
  (every operation rounded on its own: no contraction); bounds by plain selection over the absolute vertices
  with the loader's min/max (a NaN operand yields the other one, a tie keeps the earlier operand), folded in
  the order the definition gives: a, b, c per triangle, triangles of a leaf in index order, child1 then child2.
  Selection does no arithmetic, so it runs on Python floats (exact images of the float32 values, zero signs
  included).  Results are compared as uint32 views.
* ClosestRef: the reference closest-hit traversal (scene.cu:338-372, :134-241) restated over the oracle's own
  orc_ray_sphere / orc_ray_triangle / orc_ray_aabb, as anyhit_ref.py does for any-hit: a stack of (node,
  distance) pairs re-tested at pop; with both children hit and d1 < d2, child1 is pushed first (so child2,
  the far one, is popped first).  It runs over any arrays, e.g. refit ones no oracle scene exists for.
* Arrays: a shim with .arrays(), so AnyHitRef and test_gpu_trace_rays._ray_sets run over refit arrays.
* deformations(V, seed): the seeded vertex sets the CPU and GPU tests share.
* scene texts: a 400-triangle random scene with exactly known vertices, same-centroid scenes of n triangles.
"""
import ctypes as C
import math

import numpy as np

import oracle_lib as O

BIG = 1e30
F32 = np.float32


def _sel_min(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return b if b < a else a


def _sel_max(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return b if b > a else a


def _grow(box, lo, hi):
    for k in range(3):
        box[k] = _sel_min(box[k], lo[k])
        box[3 + k] = _sel_max(box[3 + k], hi[k])


def _empty():
    b = float(F32(BIG))
    return [b, b, b, -b, -b, -b]


def triangle_records(vertices):
    """(n, 9) float32 -> (n, 12) float32: p1, p2 - p1, p3 - p1, normalise(cross(p3 - p1, p2 - p1))."""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 9)
    with np.errstate(all="ignore"):
        a, e1, e2 = v[:, 0:3], v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
        x, y = e2, e1                                   # cross(p3p1, p2p1)
        n = np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                      x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], 1).astype(F32)
        s = F32(1.0) / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2], dtype=F32)
        nn = (s[:, None] * n).astype(F32)
    out = np.hstack([a, e1, e2, nn]).astype(F32)
    assert out.dtype == F32 and e1.dtype == F32 and s.dtype == F32
    return np.ascontiguousarray(out)


def refit_numpy(bvh, vertices):
    """bvh (m, 8) float32 (columns 6, 7: int32 child1, child2), vertices (n, 9) -> (triangles (n, 12),
    bvh (m, 8)) after the refit.  Children, leaf ranges and everything but the six bound columns are kept."""
    bvh = np.ascontiguousarray(bvh, F32).reshape(-1, 8)
    kids = np.ascontiguousarray(bvh[:, 6:8]).view(np.int32)
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 9)
    vl = v.astype(np.float64).tolist()                  # exact images of the float32 values
    tri_box = []
    for row in vl:
        b = _empty()
        for p in (row[0:3], row[3:6], row[6:9]):
            _grow(b, p, p)
        tri_box.append(b)
    m = bvh.shape[0]
    boxes = [None] * m
    for i in range(m - 1, -1, -1):                      # the builder appends children after their parent
        c1, c2 = int(kids[i, 0]), int(kids[i, 1])
        b = _empty()
        if c2 <= c1:
            for t in range(c2, c1):
                _grow(b, tri_box[t][0:3], tri_box[t][3:6])
        else:
            assert c1 > i and c2 > i
            for c in (c1, c2):
                _grow(b, boxes[c][0:3], boxes[c][3:6])
        boxes[i] = b
    out = bvh.copy()
    out[:, 0:6] = np.asarray(boxes, np.float64).astype(F32)
    assert np.array_equal(np.ascontiguousarray(out[:, 6:8]).view(np.int32), kids)
    return triangle_records(v), out


def key_bounds(bvh, spheres):
    """min_coord, inv_dimensions as the loader computes them (scene.cu:822-830) from the root and the spheres."""
    lo = [float(x) for x in bvh[0, 0:3]]
    hi = [float(x) for x in bvh[0, 3:6]]
    for s in np.asarray(spheres, F32).reshape(-1, 4):
        for k in range(3):
            hi[k] = _sel_max(hi[k], float(F32(s[k] + s[3])))
            lo[k] = _sel_min(lo[k], float(F32(s[k] - s[3])))
    with np.errstate(all="ignore"):
        return np.asarray(lo, F32), (F32(1.0) / np.asarray(hi, F32)).astype(F32)


class Arrays:
    """.arrays() over given arrays (spheres, triangles, bvh, ...), like an OracleScene's."""

    def __init__(self, arrays, **replace):
        self._a = dict(arrays)
        self._a.update(replace)

    def arrays(self):
        return self._a


class ClosestRef:
    def __init__(self, src):
        arr = src.arrays()
        self.L = O.lib()
        self.spheres = np.ascontiguousarray(arr["spheres"], F32).reshape(-1, 4)
        self.tris = np.ascontiguousarray(arr["triangles"], F32).reshape(-1, 12)
        self.bvh = np.ascontiguousarray(arr["bvh"], F32).reshape(-1, 8)
        kids = np.ascontiguousarray(self.bvh[:, 6:8]).view(np.int32)
        self.child1 = [int(x) for x in kids[:, 0]]
        self.child2 = [int(x) for x in kids[:, 1]]

    def query(self, ray):
        """One ray (6 float32) -> (t, index, Pn, Iv, Tt, sphere tests)."""
        L = self.L
        ray = np.ascontiguousarray(ray, F32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        sph, tri, bvh = self.spheres.ctypes.data, self.tris.ctypes.data, self.bvh.ctypes.data
        ns = self.spheres.shape[0]
        tbuf, t2 = C.c_float(), C.c_float()
        tp, tp2 = C.addressof(tbuf), C.addressof(t2)
        closest, index = float(F32(BIG)), -1
        pn = iv = tt = st = 0
        for k in range(ns):
            st += 1
            if L.orc_ray_sphere(sph + 16 * k, o, d, closest, tp):
                closest, index = tbuf.value, k
        stack = [(0, 0.0)]
        c1s, c2s = self.child1, self.child2
        while stack:
            n, dist = stack.pop()
            if dist >= closest:
                continue
            pn += 1
            c1, c2 = c1s[n], c2s[n]
            if c2 <= c1:
                for i in range(c2, c1):
                    tt += 1
                    if L.orc_ray_triangle(tri + 48 * i, o, d, closest, tp):
                        closest, index = tbuf.value, ns + i
            else:
                iv += 1
                h1 = L.orc_ray_aabb(bvh + 32 * c1, bvh + 32 * c1 + 12, o, d, closest, tp)
                h2 = L.orc_ray_aabb(bvh + 32 * c2, bvh + 32 * c2 + 12, o, d, closest, tp2)
                d1, d2 = tbuf.value, t2.value
                if h1 and h2:
                    if d1 < d2:
                        stack.append((c1, d1))
                        stack.append((c2, d2))
                    else:
                        stack.append((c2, d2))
                        stack.append((c1, d1))
                elif h1:
                    stack.append((c1, d1))
                elif h2:
                    stack.append((c2, d2))
        return closest, index, pn, iv, tt, st

    def batch(self, rays):
        """rays (n, 6) -> (t float32 (n,), index int32 (n,), counters int64 (n, 4): Pn, Iv, Tt, sphere tests)."""
        rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
        n = rays.shape[0]
        t = np.zeros(n, F32)
        idx = np.zeros(n, np.int32)
        ctr = np.zeros((n, 4), np.int64)
        for i in range(n):
            r = self.query(rays[i])
            t[i] = r[0]
            idx[i] = r[1]
            ctr[i] = r[2:]
        return t, idx, ctr


DEFORMATIONS = ("identity", "jitter", "translate_half", "collapse", "nan_vertex", "zero_snap")


def deform(V, name, seed=2024):
    """A deformed copy of V (n, 9) float32; the same (V, name, seed) always gives the same floats."""
    V = np.ascontiguousarray(V, F32).reshape(-1, 9)
    n = V.shape[0]
    rng = np.random.default_rng([seed, DEFORMATIONS.index(name)])
    P = V.reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    ext = (hi - lo).astype(F32)
    diag = F32(np.sqrt((ext.astype(np.float64) ** 2).sum()))
    W = V.copy()
    if name == "identity":
        pass
    elif name == "jitter":                              # 1 % of the diagonal, per vertex
        W = (V + (F32(0.01) * diag) * rng.normal(size=V.shape).astype(F32)).astype(F32)
    elif name == "translate_half":                      # half of the triangles moved by 10x the extent:
        move = rng.random(n) < 0.5                      # sibling boxes overlap heavily
        shift = (F32(10.0) * np.maximum(ext, F32(1e-3))).astype(F32)
        W[move] = (V[move].reshape(-1, 3, 3) + shift).reshape(-1, 9)
    elif name == "collapse":                            # zero-area triangles, zero-volume boxes
        W[:] = np.tile(((lo + hi) * F32(0.5)).astype(F32), 3)
    elif name == "nan_vertex":
        W[int(rng.integers(0, n)), 3:6] = np.nan
    elif name == "zero_snap":                           # +0 / -0 / +0 on one coordinate of a few triangles:
        for k, t in enumerate(rng.choice(n, size=min(n, 5), replace=False)):   # the tie rule decides the sign
            axis = k % 3
            W[t, axis], W[t, 3 + axis], W[t, 6 + axis] = (0.0, -0.0, 0.0) if k % 2 == 0 else (-0.0, 0.0, -0.0)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(W, F32)


HEADER = ("material white diffuse 0.8 0.8 0.8 metallicity 0.2 specular 1 1 1 roughness 0.3\n"
          "sky 0.6 0.7 0.9\n")
CAMERA = "camera position 0 0 6 forward 0 0 -1 up 0 1 0 fov 40\nimage 16 16 1 1 1\n"


def _tri_line(v9):
    return "triangle white " + " ".join("%.9g" % float(c) for c in v9) + "\n"


def random_scene(n=400, seed=11):
    """(text, vertices (n, 9) float32 in file order): small random triangles in a cube, one sphere.  %.9g
    round-trips float32, so the loader reads exactly `vertices`."""
    rng = np.random.default_rng(seed)
    c = (rng.random((n, 1, 3)) * 4 - 2).astype(F32)
    V = (c + (rng.random((n, 3, 3)) * 0.6 - 0.3).astype(F32)).astype(F32).reshape(n, 9)
    text = HEADER + "sphere white 0.5 0.25 -0.5 0.4\n" + "".join(_tri_line(v) for v in V) + CAMERA
    return text, V


def same_centroid_scene(n):
    """n triangles with one common centroid (edge_scenes.big_leaf's construction: no split separates them, so
    they end in one leaf of n) plus a ground quad.  n = 1: three triangles, the root stays a leaf; n = 5: the
    root splits once or twice; n = 63 / 64 / 65: the leaf at, and past, the 63 triangles an inline leaf ref
    holds.  The tests read the topology from the loaded scene."""
    s = HEADER
    for k in range(n):
        a = 2 * math.pi * k / n
        dx, dz = 0.5 * math.cos(a), 0.5 * math.sin(a)
        s += _tri_line((dx, 1.5, dz, -dx, 1.5, -dz, 0.0, 0.0, 0.0))
    s += "quad white -20 0 -20 -20 0 20 20 0 20 20 0 -20\n"
    return s + "camera position -4 1.5 0 forward 1 -0.1 0 up 0 1 0 fov 40\nimage 16 16 1 1 1\n"
