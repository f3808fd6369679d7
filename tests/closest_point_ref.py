"""Closest-point yardstick for rt_query_closest_point / rt_scene_closest_point -- TEST INFRASTRUCTURE ONLY.

The definition of include/rt_abi.h restated op by op in numpy float32 (every operation rounded on its own: numpy
never contracts) over Scene.arrays(): the bound, the triangle rule with its seven regions, the sphere and box rules
and the pinned walk with the shrinking bound.  Per query it returns the four outputs, the work (Pn nodes entered, Iv
internal nodes, Tt triangle tests, sphere tests), the region the accepted triangle's point lies in, how deep the stack
got, the largest leaf entered and how many tests met a primitive at exactly the best distance (decided by the index).

brute(): the same per-primitive functions over every primitive, the minimum of the key (dist2, index); brute64(): the
same formulas in float64, for the size of the float32 functions' own error.

The per-primitive functions take arrays of primitives (a leaf's triangles, or all of them), so the walk and the brute
force evaluate one text.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F32 = np.float32
BIG = F32(1e30)
INF = F32(np.inf)
INT_MAX = 2 ** 31 - 1
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "face")
LDS_ENTRIES = 8          # kStackLds: entries e >= 8 of a lane live in the kernel's global overflow buffer
INLINE_LEAF = 63         # a leaf of more triangles goes through the big-leaf table


def bound2(r):
    """max_dist -> B2 (float32)."""
    if r is None:
        return INF
    r = F32(r)
    if r < 0:
        return F32(-1.0)
    return F32(r * r) if r <= F32(1e18) else INF


def same(a, b):
    """Floats as the tests compare them: equal bits, or NaN on both sides (elementwise bool)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def triangles(p, cols, dt=F32):
    """p (3,), cols (>= 9, k): the records' columns p1.xyz, e1.xyz, e2.xyz as rows (ClosestPointRef.cols, or records.T)
    -> dist2 (k,), u, v, point (k, 3), region (k,) int; every op in dtype dt, on one coordinate of all k at a time."""
    px, py, pz = (dt(c) for c in p)
    p1x, p1y, p1z, e1x, e1y, e1z, e2x, e2y, e2z = (np.asarray(cols[i], dt) for i in range(9))
    one, zero = dt(1), dt(0)
    with np.errstate(all="ignore"):
        apx, apy, apz = px - p1x, py - p1y, pz - p1z
        bpx, bpy, bpz = apx - e1x, apy - e1y, apz - e1z
        cpx, cpy, cpz = apx - e2x, apy - e2y, apz - e2z
        d1, d2 = _dot3(e1x, e1y, e1z, apx, apy, apz), _dot3(e2x, e2y, e2z, apx, apy, apz)
        d3, d4 = _dot3(e1x, e1y, e1z, bpx, bpy, bpz), _dot3(e2x, e2y, e2z, bpx, bpy, bpz)
        d5, d6 = _dot3(e1x, e1y, e1z, cpx, cpy, cpz), _dot3(e2x, e2y, e2z, cpx, cpy, cpz)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = one / ((va + vb) + vc)
        k = p1x.shape[0]
        z, o = np.full(k, zero, dt), np.full(k, one, dt)
        cand = [(z, z), (o, z), (d1 / (d1 - d3), z), (z, o), (z, d2 / (d2 - d6)), (one - w, w), (vb * den, vc * den)]
        region = np.full(k, 6, np.int64)
        for r in range(5, -1, -1):                      # the first that applies
            region[conds[r]] = r
        u = np.choose(region, [c[0] for c in cand]).astype(dt)
        v = np.choose(region, [c[1] for c in cand]).astype(dt)
        qx, qy, qz = (p1x + u * e1x) + v * e2x, (p1y + u * e1y) + v * e2y, (p1z + u * e1z) + v * e2z
        wx, wy, wz = px - qx, py - qy, pz - qz
        dist2 = _dot3(wx, wy, wz, wx, wy, wz)
        point = np.stack([qx, qy, qz], 1)
    assert dist2.dtype == dt and point.dtype == dt and u.dtype == dt
    return dist2, u, v, point, region


def spheres(p, S, dt=F32):
    """p (3,), S (k, 4) -> dist2 (k,), point (k, 3)."""
    p = np.asarray(p, dt)
    S = np.asarray(S, dt)
    c, r = S[:, 0:3], S[:, 3]
    with np.errstate(all="ignore"):
        w = p - c
        ln = np.sqrt(_dot(w, w))
        g = ln - r
        dist2 = g * g
        point = c + (r / ln)[:, None] * w
        at = ln == 0
        if at.any():
            off = np.zeros_like(c)
            off[:, 0] = r
            point[at] = (c + off)[at]
    assert dist2.dtype == dt and point.dtype == dt
    return dist2, point


def boxes(p, lo, hi):
    """p (3,), lo, hi (k, 3) float32 -> box2 (k,)."""
    with np.errstate(all="ignore"):
        q = np.fmax(np.fmax(lo - p, p - hi), F32(0))
        b = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    assert b.dtype == F32
    return b


def accepts(dist2, i, best2, best):
    return bool(dist2 < best2 or (dist2 == best2 and i < best))


class ClosestPointRef:
    def __init__(self, src):
        """src: anything with .arrays() (rtamd.Scene, refit_ref.Arrays)."""
        arr = src.arrays()
        self.spheres = np.ascontiguousarray(arr["spheres"], F32).reshape(-1, 4)
        self.tris = np.ascontiguousarray(arr["triangles"], F32).reshape(-1, 12)
        self.cols = np.ascontiguousarray(self.tris.T)           # (12, T): one coordinate of every record per row
        bvh = np.ascontiguousarray(arr["bvh"], F32).reshape(-1, 8)
        kids = np.ascontiguousarray(bvh[:, 6:8]).view(np.int32)
        self.lo, self.hi = np.ascontiguousarray(bvh[:, 0:3]), np.ascontiguousarray(bvh[:, 3:6])
        self.child1 = [int(x) for x in kids[:, 0]]
        self.child2 = [int(x) for x in kids[:, 1]]

    def query(self, p, max_dist=None):
        """One point (3 float32) -> dict(distance, index, point (3,), uv (2,), ctr (Pn, Iv, Tt, sphere tests), region
        (-1: a sphere or a miss), depth, max_leaf, ties, tested: bit r set iff some triangle test of the walk fell into
        region r)."""
        p = np.ascontiguousarray(p, F32)
        ns = self.spheres.shape[0]
        best2, best = bound2(max_dist), INT_MAX
        pn = iv = tt = st = depth = max_leaf = ties = tested = 0
        if np.isfinite(p).all():
            if ns:
                d2 = spheres(p, self.spheres)[0]
                for k in range(ns):
                    st += 1
                    ties += best != INT_MAX and d2[k] == best2
                    if accepts(d2[k], k, best2, best):
                        best2, best = d2[k], k
            if not 0 > best2:
                c1s, c2s = self.child1, self.child2
                stack = []
                n = 0
                pn += 1
                while True:
                    c1, c2 = c1s[n], c2s[n]
                    descend = False
                    if c2 <= c1:                               # leaf: triangles [child2, child1)
                        max_leaf = max(max_leaf, c1 - c2)
                        if c1 > c2:
                            d2, _, _, _, reg = triangles(p, self.cols[:, c2:c1])
                            for r in reg:
                                tested |= 1 << int(r)
                            for j in range(c2, c1):
                                tt += 1
                                ties += best != INT_MAX and d2[j - c2] == best2
                                if accepts(d2[j - c2], ns + j, best2, best):
                                    best2, best = d2[j - c2], ns + j
                    else:
                        iv += 1
                        kids = [c1, c2]
                        a, b = boxes(p, self.lo[kids], self.hi[kids])
                        e1, e2 = not a > best2, not b > best2
                        if e1 or e2:
                            second = e2 and (not e1 or b < a)
                            if e1 and e2:
                                stack.append((c1, a) if second else (c2, b))
                                depth = max(depth, len(stack))
                            n = c2 if second else c1
                            pn += 1
                            descend = True
                    if descend:
                        continue
                    found = False
                    while stack and not found:
                        node, d = stack.pop()
                        if not d > best2:
                            n, found = node, True
                            pn += 1
                    if not found:
                        break
        out = dict(distance=BIG, index=-1, point=np.zeros(3, F32), uv=np.zeros(2, F32), region=-1)
        if best != INT_MAX:
            out["distance"], out["index"] = np.sqrt(F32(best2)), best
            if best < ns:
                out["point"] = spheres(p, self.spheres[best:best + 1])[1][0]
            else:
                _, u, v, point, region = triangles(p, self.cols[:, best - ns:best - ns + 1])
                out["point"], out["uv"], out["region"] = point[0], np.array([u[0], v[0]], F32), int(region[0])
        out.update(ctr=(pn, iv, tt, st), depth=depth, max_leaf=max_leaf, ties=int(ties), tested=tested)
        return out

    def batch(self, points, max_dist=None):
        """points (n, 3), max_dist None or (n,) -> dict of arrays: distance (n,), index (n,) int32, point (n, 3),
        uv (n, 2), ctr (n, 4) int64, region, depth, max_leaf, ties, tested (n,) int64."""
        points = np.ascontiguousarray(points, F32).reshape(-1, 3)
        n = points.shape[0]
        out = dict(distance=np.zeros(n, F32), index=np.zeros(n, np.int32), point=np.zeros((n, 3), F32),
                   uv=np.zeros((n, 2), F32), ctr=np.zeros((n, 4), np.int64), region=np.zeros(n, np.int64),
                   depth=np.zeros(n, np.int64), max_leaf=np.zeros(n, np.int64), ties=np.zeros(n, np.int64),
                   tested=np.zeros(n, np.int64))
        for i in range(n):
            r = self.query(points[i], None if max_dist is None else max_dist[i])
            for k, v in r.items():
                out[k][i] = v
        return out

    def brute(self, points, dt=F32):
        """The unpruned minimum: (dist2 (n,) in dt, index (n,) int32; -1 where nothing has a non-NaN dist2) by the key
        (dist2, index) over every primitive, for finite points."""
        points = np.ascontiguousarray(points, F32).reshape(-1, 3)
        n, ns = points.shape[0], self.spheres.shape[0]
        d2o, io = np.full(n, np.inf, dt), np.full(n, -1, np.int32)
        cols = self.cols.astype(dt)

        def one(i):
            parts = []
            if ns:
                parts.append(spheres(points[i], self.spheres, dt)[0])
            if self.tris.shape[0]:
                parts.append(triangles(points[i], cols, dt)[0])
            d2 = np.concatenate(parts)
            ok = ~np.isnan(d2)
            if ok.any():
                k = int(np.argmin(np.where(ok, d2, np.inf)))    # the first of equal minima: the smallest index
                d2o[i], io[i] = d2[k], k
        with ThreadPoolExecutor(min(4, os.cpu_count() or 1)) as pool:      # numpy releases the GIL in its loops
            list(pool.map(one, range(n)))
        return d2o, io
