"""A plain numpy float32 model of the reference's binned-SAH node decision (scene.cu:866-980) and of the
recursion on top of it (scene.cu:982-1000).  Test infrastructure: a second yardstick for the host build
(box, split and order must equal the host's) and the certificate that each case of
tests/bvh_build_cases.py reaches the path it is named for.

Every operation is a float32 operation in the reference's order, with no contraction (numpy never fuses
a multiply and an add).  min and max are the reference's (math.cuh): a NaN argument yields the other
one, and of equal values the first is kept, so the sign of a zero bound is that of its first occurrence.
Only the node's box needs that rule; bin boxes reach a decision through their areas alone, which do not
depend on the order of the min/max, so they are reduced with fmin/fmax.

A model for small and medium inputs: the full recursion is meant for a few thousand triangles, one
decision for any size.
"""
import numpy as np

F = np.float32
BINS = 8
MAX_DEPTH = 30
BIG, TINY = F(1e30), F(-1e30)


def build_input(verts):
    """verts (n, 9) float32 as written in the scene file -> per-triangle boxes (n, 3) lo and hi, grown
    from (1e30, -1e30) by p1, p2, p3 in turn, and the loader's centroids (1/3f) * ((p1 + p2) + p3)."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
    lo = np.empty((v.shape[0], 3), F)
    hi = np.empty((v.shape[0], 3), F)
    for a in range(3):
        lo[:, a] = first_min(np.concatenate([np.full((v.shape[0], 1), BIG, F), v[:, :, a]], 1), axis=1)
        hi[:, a] = first_max(np.concatenate([np.full((v.shape[0], 1), TINY, F), v[:, :, a]], 1), axis=1)
    cen = (F(1.0) / F(3.0)) * ((v[:, 0] + v[:, 1]) + v[:, 2])
    return lo, hi, cen.astype(F)


def first_min(x, axis=0):
    """Sequential min over axis: skips NaN, keeps the first of equal values (-0 == +0)."""
    x = np.asarray(x, F)
    m = np.fmin.reduce(x, axis=axis, keepdims=True)
    first = np.argmax(x == m, axis=axis)
    return np.take_along_axis(x, np.expand_dims(first, axis), axis).squeeze(axis)


def first_max(x, axis=0):
    x = np.asarray(x, F)
    m = np.fmax.reduce(x, axis=axis, keepdims=True)
    first = np.argmax(x == m, axis=axis)
    return np.take_along_axis(x, np.expand_dims(first, axis), axis).squeeze(axis)


def half_area(lo, hi):
    s = (hi - lo).astype(F)
    return F(F(F(s[0] * s[1]) + F(s[0] * s[2])) + F(s[1] * s[2]))


def loop_partition(left):
    """The reference's two-pointer loop (scene.cu:960-975) on positions 0..n-1: (order, i)."""
    a = list(range(len(left)))
    i, j = 0, len(a) - 1
    while i <= j:
        if left[a[i]]:
            i += 1
        else:
            a[i], a[j] = a[j], a[i]
            j -= 1
    return a, i


class Decision:
    """What maybe_split does with one node before it recurses."""
    __slots__ = ("lo", "hi", "count", "may_split", "skipped", "axis", "pos", "L", "a", "degenerate", "order",
                 "own_cost", "best_cost", "zero_costs", "inf_scale")


def decide(blo, bhi, cen, depth_left, start_lo=None, start_hi=None):
    """One node over the range given by blo, bhi, cen (n, 3).  order[k] = the range position whose element
    ends at position k (the identity when nothing is partitioned)."""
    n = blo.shape[0]
    d = Decision()
    with np.errstate(all="ignore"):
        d.lo = first_min(np.vstack([np.full((1, 3), BIG, F) if start_lo is None else start_lo[None], blo]))
        d.hi = first_max(np.vstack([np.full((1, 3), TINY, F) if start_hi is None else start_hi[None], bhi]))
        d.count = n
        d.may_split = n > 4 and depth_left != 0
        d.skipped = [False] * 3
        d.axis, d.pos, d.L, d.a, d.degenerate = -1, F(0), None, None, False
        d.order = list(range(n))
        d.zero_costs = 0
        d.inf_scale = [False] * 3
        if not d.may_split:
            return d
        own = F(half_area(d.lo, d.hi) * F(n))
        best = own
        for axis in range(3):
            c = cen[:, axis]
            cmin = first_min(np.concatenate([[BIG], c]))
            cmax = first_max(np.concatenate([[TINY], c]))
            if cmin == cmax:
                d.skipped[axis] = True
                continue
            scale = F(F(BINS) / F(cmax - cmin))
            d.inf_scale[axis] = bool(np.isinf(scale))
            p = ((c - cmin).astype(F) * scale).astype(F)
            # min(BINS - 1, (int)p) where that is defined; NaN -> 0, inf -> BINS - 1 (an infinite scale)
            b = np.where(p >= BINS, BINS - 1, np.where(p > 0, p, 0).astype(np.int64))
            counts = np.bincount(b, minlength=BINS)
            bin_lo = np.full((BINS, 3), BIG, F)
            bin_hi = np.full((BINS, 3), TINY, F)
            for k in range(BINS):
                if counts[k]:
                    m = b == k
                    bin_lo[k] = np.fmin(BIG, np.fmin.reduce(blo[m], axis=0))
                    bin_hi[k] = np.fmax(TINY, np.fmax.reduce(bhi[m], axis=0))
            larea, rarea, lcount = [F(0)] * (BINS - 1), [F(0)] * (BINS - 1), [0] * (BINS - 1)
            llo, lhi = np.full(3, BIG, F), np.full(3, TINY, F)
            rlo, rhi = np.full(3, BIG, F), np.full(3, TINY, F)
            lsum = 0
            for i in range(BINS - 1):
                lsum += int(counts[i])
                lcount[i] = lsum
                llo, lhi = np.fmin(llo, bin_lo[i]), np.fmax(lhi, bin_hi[i])
                larea[i] = half_area(llo, lhi)
                rlo, rhi = np.fmin(rlo, bin_lo[BINS - 1 - i]), np.fmax(rhi, bin_hi[BINS - 1 - i])
                rarea[BINS - 2 - i] = half_area(rlo, rhi)
            step = F(F(cmax - cmin) / F(BINS))
            for i in range(BINS - 1):
                cost = F(F(F(lcount[i]) * larea[i]) + F(F(n - lcount[i]) * rarea[i]))
                d.zero_costs += int(cost == 0)
                if cost != 0 and cost < best:
                    d.axis = axis
                    d.pos = F(cmin + F(step * F(i + 1)))
                    best = cost
        d.own_cost, d.best_cost = own, best
        if d.axis < 0 or best >= own:
            d.axis = -1
            return d
        left = (cen[:, d.axis] < d.pos).tolist()
        d.order, i = loop_partition(left)
        d.L = i
        d.a = i if (i == n or left[i]) else i + 1
        d.degenerate = i == 0 or i == n
        return d


class Node:
    __slots__ = ("lo", "hi", "begin", "end", "depth", "child1", "child2", "decision")

    @property
    def length(self):
        return self.end - self.begin

    @property
    def is_leaf(self):
        return self.child2 <= self.child1


def build(verts, mats, max_depth=MAX_DEPTH):
    """The reference's recursion.  Returns (nodes, perm): nodes in the reference's array order, perm the
    input index of the triangle at each final position (materials: mats[perm])."""
    blo, bhi, cen = build_input(verts)
    n = blo.shape[0]
    perm = np.arange(n)
    nodes = []

    def fresh(begin, end, depth):
        nd = Node()
        nd.begin, nd.end, nd.depth = begin, end, depth
        nd.child2, nd.child1 = begin, end
        nodes.append(nd)
        return nd

    def maybe_split(nd, depth_left):
        nonlocal blo, bhi, cen
        lo_, hi_ = nd.begin, nd.end
        d = decide(blo[lo_:hi_], bhi[lo_:hi_], cen[lo_:hi_], depth_left)
        nd.lo, nd.hi, nd.decision = d.lo, d.hi, d
        if d.axis < 0:
            return
        o = np.asarray(d.order, np.int64) + lo_
        for arr in (blo, bhi, cen, perm):
            arr[lo_:hi_] = arr[o]
        d.order = None if not d.degenerate else d.order        # kept only where a test looks at it
        if d.degenerate:
            return
        mid = lo_ + d.L
        left_index = len(nodes)
        left = fresh(lo_, mid, nd.depth + 1)
        right = fresh(mid, hi_, nd.depth + 1)
        maybe_split(left, depth_left - 1)
        maybe_split(right, depth_left - 1)
        nd.child1, nd.child2 = left_index, left_index + 1

    maybe_split(fresh(0, n, 0), max_depth)
    return nodes, perm


def node_array(nodes):
    """The (n, 8) float32 view of the node array as rtamd.Scene.arrays()['bvh'] returns it."""
    out = np.zeros((len(nodes), 8), F)
    for k, nd in enumerate(nodes):
        out[k, 0:3], out[k, 3:6] = nd.lo, nd.hi
        out[k, 6:8] = np.array([nd.child1, nd.child2], np.int32).view(F)
    return out


def render_triangles(verts):
    """The first nine floats of the ray-tracing triangle records: p1, p2 - p1, p3 - p1 (scene.cu:1029-1033)."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
    return np.concatenate([v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]], 1).astype(F)


def walk(bvh):
    """A node array (n, 8) -> per node (depth, length, is_leaf), by walking from the root."""
    ch = np.ascontiguousarray(bvh[:, 6:8]).view(np.int32)
    depth = np.zeros(len(bvh), np.int64)
    length = np.zeros(len(bvh), np.int64)
    leaf = ch[:, 1] <= ch[:, 0]
    order, stack = [], [0]
    while stack:
        x = stack.pop()
        order.append(x)
        if not leaf[x]:
            for c in (ch[x, 0], ch[x, 1]):
                depth[c] = depth[x] + 1
                stack.append(int(c))
    for x in reversed(order):
        length[x] = ch[x, 0] - ch[x, 1] if leaf[x] else length[ch[x, 0]] + length[ch[x, 1]]
    return depth, length, leaf
