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

AnyHitOrderRef restates the visit order of anyhit_kernel (csrc/rt_query.hip) over the same
predicates, so its Pn/Iv/Tt are the kernel's on every ray, occluded ones included:

  * spheres in order, return at the first accepted one (its test is counted);
  * 0 >= B: unoccluded with Pn = 0; otherwise the root is entered (Pn += 1);
  * leaf: triangles [child2, child1) in order, Tt += 1 each, occluded at the first accept; an exhausted
    leaf pops;
  * internal node (Iv += 1): (hit, t) of child1 then child2 by orc_ray_aabb(.., B); a child is entered iff
    hit and not (t >= B); child2 goes first iff it is entered and child1 is not or t2 < t1; the selected child
    is entered (Pn += 1), the other one pushed if both are entered; neither entered pops;
  * pop: an empty stack ends the ray unoccluded, otherwise the popped node is entered (Pn += 1).

The order depends on (ray, B, tree) alone.  Besides the counters it records the stack's life: the kernel
keeps entries 0..15 of a lane in LDS and entry e >= 16 in its global overflow buffer.
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


LDS_ENTRIES = 16   # kAnyStackLds: stack entries >= this one live in the kernel's overflow buffer


class AnyHitOrderRef(AnyHitRef):
    """anyhit_kernel's visit order (see the module docstring)."""

    def query(self, ray, tmax=None, entered=None):
        """One ray (6 float32) -> (occluded, Pn, Iv, Tt, sphere tests, (max depth after a push, pops from entries
        >= 16, [(entry index, node) pushed at entries >= 16])).  `entered`, a list, receives (node, how) for
        every node entered, how = "root", "selected" or "popped"."""
        L = self.L
        ray = np.ascontiguousarray(ray, np.float32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        B = float(BIG if tmax is None else bound(tmax))
        tb1, tb2 = C.c_float(), C.c_float()
        tp1, tp2 = C.addressof(tb1), C.addressof(tb2)
        pn = iv = tt = st = 0
        depth = opops = 0
        opush = []
        for k in range(self.spheres.shape[0]):
            st += 1
            if L.orc_ray_sphere(self._sph + 16 * k, o, d, B, tp1):
                return 1, pn, iv, tt, st, (depth, opops, opush)
        if 0.0 >= B:
            return 0, pn, iv, tt, st, (depth, opops, opush)
        c1s, c2s, bvh = self.child1, self.child2, self._bvh
        stack = []
        n = 0
        pn += 1
        if entered is not None:
            entered.append((n, "root"))
        while True:
            c1, c2 = c1s[n], c2s[n]
            if c2 <= c1:                                   # leaf: triangles [child2, child1)
                for i in range(c2, c1):
                    tt += 1
                    if L.orc_ray_triangle(self._tri + 48 * i, o, d, B, tp1):
                        return 1, pn, iv, tt, st, (depth, opops, opush)
            else:
                iv += 1
                e1 = bool(L.orc_ray_aabb(bvh + 32 * c1, bvh + 32 * c1 + 12, o, d, B, tp1)) and not (tb1.value >= B)
                e2 = bool(L.orc_ray_aabb(bvh + 32 * c2, bvh + 32 * c2 + 12, o, d, B, tp2)) and not (tb2.value >= B)
                if e1 or e2:
                    first2 = e2 and (not e1 or tb2.value < tb1.value)
                    n, far = (c2, c1) if first2 else (c1, c2)
                    if e1 and e2:
                        if len(stack) >= LDS_ENTRIES:
                            opush.append((len(stack), far))
                        stack.append(far)
                        depth = max(depth, len(stack))
                    pn += 1
                    if entered is not None:
                        entered.append((n, "selected"))
                    continue
            if not stack:
                return 0, pn, iv, tt, st, (depth, opops, opush)
            if len(stack) > LDS_ENTRIES:                   # the top is entry len - 1 >= 16
                opops += 1
            n = stack.pop()
            pn += 1
            if entered is not None:
                entered.append((n, "popped"))

    def batch(self, rays, tmax=None):
        """rays (n, 6), tmax None or (n,) -> (mask bool (n,), counters int64 (n, 4): Pn, Iv, Tt, sphere tests,
        max depth int64 (n,), overflow pops int64 (n,), overflow pushes: list of n lists of (entry, node))."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        mask = np.zeros(n, np.bool_)
        ctr = np.zeros((n, 4), np.int64)
        depth = np.zeros(n, np.int64)
        opops = np.zeros(n, np.int64)
        opush = []
        for i in range(n):
            r = self.query(rays[i], None if tmax is None else tmax[i])
            mask[i] = bool(r[0])
            ctr[i] = r[1:5]
            depth[i], opops[i] = r[5][0], r[5][1]
            opush.append(r[5][2])
        return mask, ctr, depth, opops, opush
