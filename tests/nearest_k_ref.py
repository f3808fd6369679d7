"""Range-query yardstick for rt_query_nearest_k / rt_scene_nearest_k -- TEST INFRASTRUCTURE ONLY.

The definition of include/rt_abi.h in numpy float32 over Scene.arrays(), on closest_point_ref.py's per-primitive and
box functions (one text for the bound, the triangle, sphere and box rules): the set H by the predicates with the bound
held, the sort by the key (dist2 bits, index), the outputs with their padding, the counters of the full walk (Pn nodes
entered, Iv internal nodes, Tt triangle tests, sphere tests), and -- in the kernel's order, the nearer child first, a tie
to child1 -- how deep the stack of refs gets and the largest leaf entered.

brute(): the same per-primitive functions over every primitive, the set {dist2 <= B2}; for each of its members that H
lacks, pruned_by() names the ancestor node whose float box2 exceeds B2 (relation 3 of rt_abi.h: the only way the two
sets can differ).
"""
import numpy as np

from closest_point_ref import BIG, F32, ClosestPointRef, bound2, boxes, spheres, triangles

ANY_LDS_ENTRIES = 16     # kAnyStackLds: entries e >= 16 of a lane live in the kernel's global overflow buffer
K_MAX = 64
FIELDS = ("distance", "index", "point", "count")


def key_order(d2, idx):
    """The order of the key (dist2 bits as uint32, index) ascending."""
    bits = np.ascontiguousarray(d2, F32).view(np.uint32).astype(np.int64)
    return np.lexsort((np.asarray(idx, np.int64), bits))


class NearestKRef(ClosestPointRef):
    def __init__(self, src):
        super().__init__(src)
        n = len(self.child1)
        self.c1, self.c2 = np.array(self.child1, np.int64), np.array(self.child2, np.int64)
        self.parent = [-1] * n
        self.leaf_of = np.full(self.tris.shape[0], -1, np.int64)
        for i in range(n):
            c1, c2 = self.child1[i], self.child2[i]
            if c2 <= c1:
                self.leaf_of[c2:c1] = i
            else:
                self.parent[c1] = self.parent[c2] = i

    def members(self, p, max_dist=None):
        """One point -> dict(d2, index: H sorted by the key; ctr (Pn, Iv, Tt, sphere tests); depth, max_leaf).
        H and the counters do not depend on the order, so the tree is walked a level at a time, every entered node of
        a level in one numpy call.  The kernel's order (the nearer child first, a tie to child1, the other one pushed
        iff both are entered) is carried along as each node's stack height on entry: the first child is entered one
        entry higher than its parent when the other one was pushed, the pushed one at its parent's height."""
        p = np.ascontiguousarray(p, F32)
        ns = self.spheres.shape[0]
        b2 = bound2(max_dist)
        d2s, ids, entered = [], [], []
        pn = iv = tt = st = depth = max_leaf = 0
        if np.isfinite(p).all():
            if ns:
                d2 = spheres(p, self.spheres)[0]
                st += ns
                ok = d2 <= b2
                d2s.append(d2[ok])
                ids.append(np.nonzero(ok)[0])
            if not 0 > b2:
                nodes, height = np.zeros(1, np.int64), np.zeros(1, np.int64)
                while nodes.size:
                    pn += nodes.size
                    c1, c2 = self.c1[nodes], self.c2[nodes]
                    leaf = c2 <= c1
                    size = (c1 - c2)[leaf]
                    if size.size and size.max() > 0:           # leaves: triangles [child2, child1)
                        max_leaf = max(max_leaf, int(size.max()))
                        first = np.repeat(c2[leaf] - (np.cumsum(size) - size), size)
                        entered.append(first + np.arange(int(size.sum())))
                    k1, k2, h = c1[~leaf], c2[~leaf], height[~leaf]
                    iv += k1.size
                    if not k1.size:
                        break
                    a, b = boxes(p, self.lo[k1], self.hi[k1]), boxes(p, self.lo[k2], self.hi[k2])
                    e1, e2 = ~(a > b2), ~(b > b2)
                    second = e2 & (~e1 | (b < a))
                    both = e1 & e2
                    if both.any():
                        depth = max(depth, int(h[both].max()) + 1)
                    h1 = np.where(both & ~second, h + 1, h)    # child1 first: entered above the pushed child2
                    h2 = np.where(both & second, h + 1, h)
                    nodes = np.concatenate([k1[e1], k2[e2]])
                    height = np.concatenate([h1[e1], h2[e2]])
                if entered:                                    # every triangle of the entered leaves, in one call
                    tri = np.concatenate(entered)
                    d2 = triangles(p, self.cols[:, tri])[0]
                    tt += tri.size
                    with np.errstate(invalid="ignore"):
                        ok = d2 <= b2                          # a NaN dist2 never qualifies
                    d2s.append(d2[ok])
                    ids.append(ns + tri[ok])
        d2 = np.concatenate(d2s).astype(F32) if d2s else np.zeros(0, F32)
        idx = np.concatenate(ids).astype(np.int64) if ids else np.zeros(0, np.int64)
        o = key_order(d2, idx)
        return dict(d2=d2[o], index=idx[o], ctr=(pn, iv, tt, st), depth=depth, max_leaf=max_leaf)

    def walk(self, points, max_dist=None):
        """points (n, 3), max_dist None or (n,) -> the list of members() results."""
        points = np.ascontiguousarray(points, F32).reshape(-1, 3)
        return [self.members(points[i], None if max_dist is None else max_dist[i]) for i in range(points.shape[0])]

    def rows(self, points, walked, k):
        """The outputs for k from walk()'s results: dict(distance (n, k), index (n, k) int32, point (n, k, 3),
        count (n,) int32, ctr (n, 4) int64, depth, max_leaf (n,), tie (n,) bool: two kept neighbours with equal dist2)."""
        points = np.ascontiguousarray(points, F32).reshape(-1, 3)
        n, ns = points.shape[0], self.spheres.shape[0]
        out = dict(distance=np.full((n, k), BIG, F32), index=np.full((n, k), -1, np.int32), point=np.zeros((n, k, 3), F32),
                   count=np.zeros(n, np.int32), ctr=np.zeros((n, 4), np.int64), depth=np.zeros(n, np.int64),
                   max_leaf=np.zeros(n, np.int64), tie=np.zeros(n, bool))
        for i, w in enumerate(walked):
            m = min(k, w["index"].shape[0])
            out["count"][i] = w["index"].shape[0]
            out["ctr"][i], out["depth"][i], out["max_leaf"][i] = w["ctr"], w["depth"], w["max_leaf"]
            if m == 0:
                continue
            idx, d2 = w["index"][:m], w["d2"][:m]
            out["distance"][i, :m] = np.sqrt(d2)
            out["index"][i, :m] = idx
            out["tie"][i] = bool((d2[1:].view(np.uint32) == d2[:-1].view(np.uint32)).any())
            sph = idx < ns
            if sph.any():
                out["point"][i, :m][sph] = spheres(points[i], self.spheres[idx[sph]])[1]
            if (~sph).any():
                out["point"][i, :m][~sph] = triangles(points[i], self.cols[:, idx[~sph] - ns])[3]
        return out

    def brute(self, p, max_dist=None):
        """The indices of {dist2 <= B2} over every primitive under the same functions, ascending; a non-finite point
        has none."""
        p = np.ascontiguousarray(p, F32)
        if not np.isfinite(p).all():
            return np.zeros(0, np.int64)
        b2 = bound2(max_dist)
        ns = self.spheres.shape[0]
        parts = []
        if ns:
            parts.append(spheres(p, self.spheres)[0])
        if self.tris.shape[0]:
            parts.append(triangles(p, self.cols)[0])
        with np.errstate(invalid="ignore"):
            return np.nonzero(np.concatenate(parts) <= b2)[0]

    def pruned_by(self, p, max_dist, prim):
        """For triangle index `prim` (>= S) outside H: (node, box2) of the outermost ancestor (the leaf included, the
        root excluded: the root is entered iff !(0 > B2)) whose box2 > B2, or None if there is none."""
        p = np.ascontiguousarray(p, F32)
        b2 = bound2(max_dist)
        n = int(self.leaf_of[prim - self.spheres.shape[0]])
        found = None
        while n > 0:
            d = boxes(p, self.lo[n:n + 1], self.hi[n:n + 1])[0]
            if d > b2:
                found = (n, d)
            n = self.parent[n]
        return found
