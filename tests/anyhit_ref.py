"""Any-hit yardstick for rt_query_occluded -- TEST INFRASTRUCTURE ONLY.

occluded(ray, tmax) is the reference traversal (scene.cu:338-372, :134-241) with `closest` held at the
bound B and never updated; 1 iff some primitive is accepted.  B = tmax if tmax <= 1e30, else 1e30 (so
NaN and +inf give 1e30).  Spelled out, with every predicate evaluated by the oracle's own functions:

  * each sphere: orc_ray_sphere(.., closest = B);
  * the root is entered iff !(0 >= B);
  * in a leaf, each triangle: orc_ray_triangle(.., closest = B);
  * at an internal node, a child is entered iff orc_ray_aabb(child, .., tmax = B) and !(entry >= B).

The bound never shrinks, so which nodes are entered depends on (ray, B, node) only: the visit order below
(a plain stack) is as good as any.  Besides the answer it returns the work of the full traversal up to the
first accepted primitive: Pn (nodes entered), Iv (internal nodes), Tt (triangle tests) and sphere tests;
on unoccluded rays these are order-independent.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

BIG = np.float32(1e30)


def bound(tmax):
    """B of a caller's tmax (float32 compare, as the kernel's)."""
    t = np.float32(tmax)
    return t if t <= BIG else BIG


class AnyHitRef:
    def __init__(self, orc):
        arr = orc.arrays()
        self.L = O.lib()
        self.spheres = np.ascontiguousarray(arr["spheres"], np.float32).reshape(-1, 4)
        self.tris = np.ascontiguousarray(arr["triangles"], np.float32).reshape(-1, 12)
        self.bvh = np.ascontiguousarray(arr["bvh"], np.float32).reshape(-1, 8)
        kids = np.ascontiguousarray(self.bvh[:, 6:8]).view(np.int32)      # child1, child2
        self.child1 = [int(v) for v in kids[:, 0]]
        self.child2 = [int(v) for v in kids[:, 1]]
        self._sph = self.spheres.ctypes.data
        self._tri = self.tris.ctypes.data
        self._bvh = self.bvh.ctypes.data

    def query(self, ray, tmax=None):
        """One ray (6 float32) -> (occluded, Pn, Iv, Tt, sphere tests)."""
        L = self.L
        ray = np.ascontiguousarray(ray, np.float32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        B = float(BIG if tmax is None else bound(tmax))
        tbuf = C.c_float()
        tp = C.addressof(tbuf)
        pn = iv = tt = st = 0
        for k in range(self.spheres.shape[0]):
            st += 1
            if L.orc_ray_sphere(self._sph + 16 * k, o, d, B, tp):
                return 1, pn, iv, tt, st
        if 0.0 >= B:
            return 0, pn, iv, tt, st
        stack = [0]
        c1s, c2s, bvh = self.child1, self.child2, self._bvh
        while stack:
            n = stack.pop()
            pn += 1
            c1, c2 = c1s[n], c2s[n]
            if c2 <= c1:                                   # leaf: triangles [child2, child1)
                for i in range(c2, c1):
                    tt += 1
                    if L.orc_ray_triangle(self._tri + 48 * i, o, d, B, tp):
                        return 1, pn, iv, tt, st
            else:
                iv += 1
                for c in (c1, c2):
                    if L.orc_ray_aabb(bvh + 32 * c, bvh + 32 * c + 12, o, d, B, tp) and not (tbuf.value >= B):
                        stack.append(c)
        return 0, pn, iv, tt, st

    def batch(self, rays, tmax=None):
        """rays (n, 6), tmax None or (n,) -> (mask bool (n,), counters int64 (n, 4): Pn, Iv, Tt, sphere tests)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        mask = np.zeros(n, np.bool_)
        ctr = np.zeros((n, 4), np.int64)
        for i in range(n):
            r = self.query(rays[i], None if tmax is None else tmax[i])
            mask[i] = bool(r[0])
            ctr[i] = r[1:]
        return mask, ctr
