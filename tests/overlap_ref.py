"""Box-overlap yardstick for rt_query_overlap_box / rt_scene_overlap_box -- TEST INFRASTRUCTURE ONLY.

host/box_overlap_math.h restated operation for operation in numpy float32 (every operation rounded on its own: numpy
never contracts) over Scene.arrays(): the valid-box rule, boxes_meet, the 13-axis triangle test and the sphere test;
the set H a level at a time with the full walk's counters (Pn nodes entered, Iv internal nodes, Tt triangle tests,
sphere tests), the stack height on entry in the pinned order and the largest leaf entered; the pinned any-only walk,
which stops at its first member, with its counters; the brute-force set, and for each of its members that H lacks the
ancestor node whose box fails boxes_meet.

triangle_gap64(): the triangle test once more in float64 with normalised axes (zero axes skipped), giving the largest
signed gap over the axes -- positive: separated by that much, negative: every axis overlaps at least that deep.  It is
used only to decide pairs far from the boundary (test_overlap_host.py's meaning test).
"""
import numpy as np

from closest_point_ref import F32, ClosestPointRef

ANY_LDS_ENTRIES = 16     # kAnyStackLds: entries e >= 16 of a lane live in the kernel's global overflow buffer
K_MAX = 64
FIELDS = ("index", "count", "any")


def valid_box(b):
    """b (6,) float32 -> all six finite and lo <= hi on every axis."""
    b = np.asarray(b, F32)
    return bool(np.isfinite(b).all() and (b[0:3] <= b[3:6]).all())


def boxes_meet(nlo, nhi, qlo, qhi):
    """nlo, nhi (k, 3); qlo, qhi (3,) -> (k,) bool.  Comparisons only, closed."""
    return ((nlo <= qhi) & (qlo <= nhi)).all(1)


def _min3(a, b, c):
    return np.fmin(np.fmin(a, b), c)


def _max3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def _edge_axis(a1, a2, p0, q0, p1, q1, p2, q2, lo1, hi1, lo2, hi2):
    t0, t1, t2 = a1 * p0 + a2 * q0, a1 * p1 + a2 * q1, a1 * p2 + a2 * q2
    b1l, b1h, b2l, b2h = a1 * lo1, a1 * hi1, a2 * lo2, a2 * hi2
    bmin = np.fmin(b1l, b1h) + np.fmin(b2l, b2h)
    bmax = np.fmax(b1l, b1h) + np.fmax(b2l, b2h)
    return (_min3(t0, t1, t2) > bmax) | (_max3(t0, t1, t2) < bmin)


def _edge_axes(f, v0, v1, v2, lo, hi):
    X, Y, Z = 0, 1, 2
    sx = _edge_axis(f[Z], -f[Y], v0[Y], v0[Z], v1[Y], v1[Z], v2[Y], v2[Z], lo[Y], hi[Y], lo[Z], hi[Z])
    sy = _edge_axis(-f[Z], f[X], v0[X], v0[Z], v1[X], v1[Z], v2[X], v2[Z], lo[X], hi[X], lo[Z], hi[Z])
    sz = _edge_axis(f[Y], -f[X], v0[X], v0[Y], v1[X], v1[Y], v2[X], v2[Y], lo[X], hi[X], lo[Y], hi[Y])
    return sx | sy | sz


def triangle_meets(cols, qlo, qhi):
    """cols (>= 9, k): the records' columns p1.xyz, e1.xyz, e2.xyz as rows; qlo, qhi (3,) float32 -> (k,) bool."""
    lo, hi = [F32(c) for c in qlo], [F32(c) for c in qhi]
    v0 = [np.asarray(cols[i], F32) for i in range(0, 3)]
    e1 = [np.asarray(cols[i], F32) for i in range(3, 6)]
    e2 = [np.asarray(cols[i], F32) for i in range(6, 9)]
    with np.errstate(all="ignore"):
        v1 = [v0[c] + e1[c] for c in range(3)]
        v2 = [v0[c] + e2[c] for c in range(3)]
        sep = np.zeros(v0[0].shape[0], bool)
        for c in range(3):                                  # axes 1-3
            sep |= (_min3(v0[c], v1[c], v2[c]) > hi[c]) | (_max3(v0[c], v1[c], v2[c]) < lo[c])
        m = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]   # axis 4
        s = (m[0] * v0[0] + m[1] * v0[1]) + m[2] * v0[2]
        a, b = [m[c] * lo[c] for c in range(3)], [m[c] * hi[c] for c in range(3)]
        bmin = (np.fmin(a[0], b[0]) + np.fmin(a[1], b[1])) + np.fmin(a[2], b[2])
        bmax = (np.fmax(a[0], b[0]) + np.fmax(a[1], b[1])) + np.fmax(a[2], b[2])
        sep |= (s < bmin) | (s > bmax)
        e3 = [e2[c] - e1[c] for c in range(3)]
        for f in (e1, e2, e3):                              # axes 5-13
            sep |= _edge_axes(f, v0, v1, v2, lo, hi)
    assert s.dtype == F32 and bmin.dtype == F32 and v1[0].dtype == F32
    return ~sep


def sphere_meets(S, qlo, qhi):
    """S (k, 4) float32; qlo, qhi (3,) -> (k,) bool."""
    S = np.asarray(S, F32)
    qlo, qhi = np.asarray(qlo, F32), np.asarray(qhi, F32)
    c, r = S[:, 0:3], S[:, 3]
    with np.errstate(all="ignore"):
        q = np.fmax(np.fmax(qlo - c, c - qhi), F32(0))       # cp::box2(c, lo, hi)
        near2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        f = np.fmax(np.abs(c - qlo), np.abs(qhi - c))
        far2 = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]
        r2 = r * r
        ok = (near2 <= r2) & (far2 >= r2)
    assert near2.dtype == F32 and far2.dtype == F32
    return ok


def triangle_gap64(cols, qlo, qhi):
    """The 13 axes in float64, each normalised (a zero axis is skipped) -> (k,) float64: the largest over the axes of
    max(tmin - bmax, bmin - tmax).  > 0: separated by that distance on some axis; < 0: every axis overlaps at least
    that deep."""
    D = np.float64
    lo, hi = np.asarray(qlo, D), np.asarray(qhi, D)
    v0 = np.stack([np.asarray(cols[i], D) for i in range(0, 3)], 1)
    e1 = np.stack([np.asarray(cols[i], D) for i in range(3, 6)], 1)
    e2 = np.stack([np.asarray(cols[i], D) for i in range(6, 9)], 1)
    # the float32 vertices the definition uses, then everything in float64
    v1 = (v0.astype(F32) + e1.astype(F32)).astype(D)
    v2 = (v0.astype(F32) + e2.astype(F32)).astype(D)
    k = v0.shape[0]
    gap = np.full(k, -np.inf)
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[i], (k, 3)) for i in range(3)] + [np.cross(e1, e2)]
    for f in (e1, e2, e2 - e1):
        axes += [np.cross(f, np.broadcast_to(unit[i], (k, 3))) for i in range(3)]
    with np.errstate(all="ignore"):
        for a in axes:
            ln = np.sqrt((a * a).sum(1))
            ok = ln > 0
            a = a / np.where(ok, ln, 1.0)[:, None]
            t = np.stack([(a * v).sum(1) for v in (v0, v1, v2)], 1)
            bmin = np.minimum(a * lo, a * hi).sum(1)
            bmax = np.maximum(a * lo, a * hi).sum(1)
            g = np.maximum(t.min(1) - bmax, bmin - t.max(1))
            gap = np.where(ok, np.maximum(gap, g), gap)
    return gap


class OverlapRef(ClosestPointRef):
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

    def members(self, box):
        """One box (6,) -> dict(index: H ascending; ctr (Pn, Iv, Tt, sphere tests) of the full walk; depth: the most
        entries on the stack in the pinned order; max_leaf).  H and these counters do not depend on the order, so the
        tree is walked a level at a time.  The pinned order (child1 first if it meets, child2 pushed when both meet) is
        carried along as each node's stack height on entry."""
        box = np.ascontiguousarray(box, F32)
        ns = self.spheres.shape[0]
        ids, entered = [], []
        pn = iv = tt = st = depth = max_leaf = 0
        if valid_box(box):
            qlo, qhi = box[0:3], box[3:6]
            if ns:
                st += ns
                ids.append(np.nonzero(sphere_meets(self.spheres, qlo, qhi))[0])
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
                m1 = boxes_meet(self.lo[k1], self.hi[k1], qlo, qhi)
                m2 = boxes_meet(self.lo[k2], self.hi[k2], qlo, qhi)
                both = m1 & m2
                if both.any():
                    depth = max(depth, int(h[both].max()) + 1)
                h1 = np.where(both, h + 1, h)               # child1 first: entered above the pushed child2
                nodes = np.concatenate([k1[m1], k2[m2]])
                height = np.concatenate([h1[m1], h[m2]])
            if entered:                                     # every triangle of the entered leaves, in one call
                tri = np.concatenate(entered)
                tt += tri.size
                ids.append(ns + tri[triangle_meets(self.cols[:, tri], qlo, qhi)])
        idx = np.sort(np.concatenate(ids).astype(np.int64)) if ids else np.zeros(0, np.int64)
        return dict(index=idx, ctr=(pn, iv, tt, st), depth=depth, max_leaf=max_leaf)

    def any_walk(self, box):
        """The pinned any-only walk of one box -> (any, (Pn, Iv, Tt, sphere tests)): spheres in order; the root; a
        leaf's triangles in order; child1 entered if it meets, else child2, child2 pushed when both meet; a pop enters
        the node; the first member ends the walk."""
        box = np.ascontiguousarray(box, F32)
        pn = iv = tt = st = 0
        if not valid_box(box):
            return 0, (0, 0, 0, 0)
        qlo, qhi = box[0:3], box[3:6]
        ns = self.spheres.shape[0]
        if ns:
            hit = np.nonzero(sphere_meets(self.spheres, qlo, qhi))[0]
            if hit.size:
                return 1, (0, 0, 0, int(hit[0]) + 1)
            st = ns
        stack = [0]
        while stack:
            n = stack.pop()
            pn += 1
            c1, c2 = self.child1[n], self.child2[n]
            if c2 <= c1:
                if c1 > c2:
                    hit = np.nonzero(triangle_meets(self.cols[:, c2:c1], qlo, qhi))[0]
                    if hit.size:
                        return 1, (pn, iv, tt + int(hit[0]) + 1, st)
                    tt += c1 - c2
                continue
            iv += 1
            kids = np.array([c1, c2])
            m = boxes_meet(self.lo[kids], self.hi[kids], qlo, qhi)
            if m[1]:
                stack.append(c2)
            if m[0]:
                stack.append(c1)
        return 0, (pn, iv, tt, st)

    def walk(self, boxes):
        boxes = np.ascontiguousarray(boxes, F32).reshape(-1, 6)
        return [self.members(b) for b in boxes]

    def rows(self, walked, k):
        """The outputs for k from walk()'s results: dict(index (n, k) int32, count (n,) int32, any (n,) uint8, ctr (n, 4)
        int64, depth, max_leaf (n,))."""
        n = len(walked)
        out = dict(index=np.full((n, k), -1, np.int32), count=np.zeros(n, np.int32), any=np.zeros(n, np.uint8),
                   ctr=np.zeros((n, 4), np.int64), depth=np.zeros(n, np.int64), max_leaf=np.zeros(n, np.int64))
        for i, w in enumerate(walked):
            m = min(k, w["index"].shape[0])
            out["count"][i] = w["index"].shape[0]
            out["any"][i] = 1 if w["index"].shape[0] else 0
            out["ctr"][i], out["depth"][i], out["max_leaf"][i] = w["ctr"], w["depth"], w["max_leaf"]
            out["index"][i, :m] = w["index"][:m]
        return out

    def brute(self, box):
        """The indices of every primitive that passes sphere_meets / triangle_meets, ascending; none for a box that is
        not valid."""
        box = np.ascontiguousarray(box, F32)
        if not valid_box(box):
            return np.zeros(0, np.int64)
        qlo, qhi = box[0:3], box[3:6]
        ns = self.spheres.shape[0]
        parts = []
        if ns:
            parts.append(np.nonzero(sphere_meets(self.spheres, qlo, qhi))[0])
        if self.tris.shape[0]:
            parts.append(ns + np.nonzero(triangle_meets(self.cols, qlo, qhi))[0])
        return np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)

    def failed_ancestor(self, box, prim):
        """For triangle index `prim` (>= S) outside H: the outermost ancestor node (the leaf included, the root excluded:
        the root is always entered) whose box fails boxes_meet, or None if there is none."""
        box = np.ascontiguousarray(box, F32)
        n = int(self.leaf_of[prim - self.spheres.shape[0]])
        found = None
        while n > 0:
            if not boxes_meet(self.lo[n:n + 1], self.hi[n:n + 1], box[0:3], box[3:6])[0]:
                found = n
            n = self.parent[n]
        return found
