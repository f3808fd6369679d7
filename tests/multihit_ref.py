"""Multi-hit yardstick for rt_query_multi_hit / rt_scene_multi_hit -- TEST INFRASTRUCTURE ONLY.

H(ray, tmax) is the set of primitives the reference traversal (scene.cu:338-372, :134-241) accepts with `closest`
held at the bound B and never updated, with NO early return; B = tmax if tmax <= 1e30, else 1e30.  The predicates are
AnyHitRef's, each evaluated by the oracle's own function:

  * each sphere k: orc_ray_sphere(.., closest = B); accepted -> the hit (t, k);
  * the root is entered iff !(0 >= B);
  * in a leaf, each triangle j: orc_ray_triangle(.., closest = B); accepted -> (t, sphere_count + j);
  * at an internal node, a child is entered iff orc_ray_aabb(child, .., tmax = B) and !(entry >= B).

The bound never shrinks, so H and the work -- Pn (nodes entered), Iv (internal nodes), Tt (triangle tests), sphere
tests -- depend on (ray, B, tree) alone, not on the visit order.  The walk below takes multihit_kernel's order (near
child first, the far one pushed; anyhit_ref.AnyHitOrderRef's rule) only to record how deep that kernel's stack gets:
it keeps entries 0..15 of a lane in LDS and entry e >= 16 in its global overflow buffer.

Hits are ordered by the key (t', index): t' = t's float32 bits as an unsigned integer, every NaN as 0x7FC00000.
"""
import ctypes as C

import numpy as np

from anyhit_ref import BIG, LDS_ENTRIES, AnyHitRef, bound

NAN_KEY = 0x7FC00000


def key(t):
    """t' of a float32 t."""
    t = np.float32(t)
    return NAN_KEY if t != t else int(t.view(np.uint32))


def same(a, b):
    """Floats as the tests compare them: equal bits, or NaN on both sides (elementwise bool)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


class MultiHitRef(AnyHitRef):
    def query(self, ray, tmax=None):
        """One ray (6 float32) -> (records: [(t float32, index)] sorted by the key, count, Pn, Iv, Tt, sphere tests,
        max stack depth of the kernel's order)."""
        L = self.L
        ray = np.ascontiguousarray(ray, np.float32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        B = float(BIG if tmax is None else bound(tmax))
        tb1, tb2 = C.c_float(), C.c_float()
        tp1, tp2 = C.addressof(tb1), C.addressof(tb2)
        ns = self.spheres.shape[0]
        pn = iv = tt = st = depth = 0
        hits = []
        for k in range(ns):
            st += 1
            if L.orc_ray_sphere(self._sph + 16 * k, o, d, B, tp1):
                hits.append((np.float32(tb1.value), k))
        if not 0.0 >= B:
            c1s, c2s, bvh = self.child1, self.child2, self._bvh
            stack = []
            n = 0
            pn += 1
            while True:
                c1, c2 = c1s[n], c2s[n]
                descend = False
                if c2 <= c1:                                   # leaf: triangles [child2, child1)
                    for i in range(c2, c1):
                        tt += 1
                        if L.orc_ray_triangle(self._tri + 48 * i, o, d, B, tp1):
                            hits.append((np.float32(tb1.value), ns + i))
                else:
                    iv += 1
                    e1 = bool(L.orc_ray_aabb(bvh + 32 * c1, bvh + 32 * c1 + 12, o, d, B, tp1)) and not (tb1.value >= B)
                    e2 = bool(L.orc_ray_aabb(bvh + 32 * c2, bvh + 32 * c2 + 12, o, d, B, tp2)) and not (tb2.value >= B)
                    if e1 or e2:
                        first2 = e2 and (not e1 or tb2.value < tb1.value)
                        n, far = (c2, c1) if first2 else (c1, c2)
                        if e1 and e2:
                            stack.append(far)
                            depth = max(depth, len(stack))
                        pn += 1
                        descend = True
                if descend:
                    continue
                if not stack:
                    break
                n = stack.pop()
                pn += 1
        hits.sort(key=lambda h: (key(h[0]), h[1]))
        return hits, len(hits), pn, iv, tt, st, depth

    def batch(self, rays, tmax=None):
        """rays (n, 6), tmax None or (n,) -> (records: list of n sorted lists, count int32 (n,), counters int64
        (n, 4): Pn, Iv, Tt, sphere tests, max depth int64 (n,))."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        recs = []
        count = np.zeros(n, np.int32)
        ctr = np.zeros((n, 4), np.int64)
        depth = np.zeros(n, np.int64)
        for i in range(n):
            r = self.query(rays[i], None if tmax is None else tmax[i])
            recs.append(r[0])
            count[i] = r[1]
            ctr[i] = r[2:6]
            depth[i] = r[6]
        return recs, count, ctr, depth


def rows(recs, k):
    """The (t (n, k) float32, index (n, k) int32) rows of sorted records: the first k, padded with (1e30, -1)."""
    n = len(recs)
    t = np.full((n, k), BIG, np.float32)
    idx = np.full((n, k), -1, np.int32)
    for i, r in enumerate(recs):
        m = min(len(r), k)
        if m:
            t[i, :m] = [h[0] for h in r[:m]]
            idx[i, :m] = [h[1] for h in r[:m]]
    return t, idx


def differing_rows(got, want, k):
    """Rows where (t, index, count) got != want; got and want are (t, index, count) triples."""
    bad = ~same(got[0], want[0]).reshape(-1, k).all(1) | (got[1] != want[1]).reshape(-1, k).any(1) | (got[2] != want[2])
    return np.nonzero(bad)[0]


def kept_ties(recs, k):
    """How many neighbouring kept records (within the first k of a row) share t' under different indices."""
    ties = 0
    for r in recs:
        for a, b in zip(r[:k], r[1:k]):
            ties += key(a[0]) == key(b[0]) and a[1] != b[1]
    return ties
