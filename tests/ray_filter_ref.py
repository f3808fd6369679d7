"""Yardstick of the filtered ray queries (rt_abi.h) -- TEST INFRASTRUCTURE ONLY.

numpy float32 over Scene.arrays(), with the triangle and box tests evaluated by the oracle's own orc_ray_triangle and
orc_ray_aabb and the sphere's two roots restated here in numpy float32 (each operation rounded once).  Nothing of the
product's filter code is used.

The filter of ray i (members None = not given):
  lo = tmin if tmin > kEps else kEps;  B = tmax if tmax <= 1e30 else 1e30;  rm = mask or 0xFFFFFFFF;
  eligible(p) = p != skip and (M[p] & rm) != 0, M[p] = 0xFFFFFFFF without primitive masks.
  triangle j under a bound c: orc_ray_triangle(.., closest = c) and not (t < lo) and eligible(S + j).
  sphere k under a bound c: the near root mhb - hs if t < c and not (t < lo), else the far root mhb + hs under the same
  test; and eligible(k).

closest(): the pinned near-first walk with the shrinking bound -- spheres in order; 0 >= closest ends the ray with
Pn = 0, otherwise the root is entered; a leaf's triangles in order; at an internal node (Iv + 1) orc_ray_aabb of child1
then child2 with tmax = closest, a child entered iff hit and not (entry >= closest), child2 first iff it is entered and
(child1 is not or t2 < t1), the selected child entered (Pn + 1), the other pushed with its entry if both are; a pop
discards entries with entry >= the current closest without counting and enters the first survivor (Pn + 1).
anyhit(): AnyHitOrderRef's walk (tests/anyhit_ref.py) with the bound held at B and these acceptance tests.
Both also return the stack's life: (max depth after a push, pops from entries >= the kernel's LDS entries, discarded pops).
brute(): every eligible primitive accepted under the bound B, no tree: [(t, p)].
"""
import ctypes as C

import numpy as np

import oracle_lib as O

F = np.float32
K_EPS = np.array([0x3BA3D70B], np.uint32).view(np.float32)[0]      # 0x1.47ae16p-8f: (double)t < 0.005 <=> t < K_EPS
BIG = F(1e30)
ALL = 0xFFFFFFFF
CLOSEST_LDS = 8    # kStackLds: (ref, entry) pairs per lane in LDS of filtered_closest_kernel
ANYHIT_LDS = 16    # kAnyStackLds: refs per lane in LDS of filtered_anyhit_kernel


def lower(tmin):
    if tmin is None:
        return K_EPS
    t = F(tmin)
    return t if t > K_EPS else K_EPS


def upper(tmax):
    if tmax is None:
        return BIG
    t = F(tmax)
    return t if t <= BIG else BIG


def sphere_roots(sph, ray):
    """(has roots, near root, far root) of one sphere (4 float32) and one ray (6 float32), float32 throughout."""
    with np.errstate(all="ignore"):
        off = sph[:3] - ray[:3]
        d = ray[3:6]
        mhb = (off[0] * d[0] + off[1] * d[1]) + off[2] * d[2]
        qc = ((off[0] * off[0] + off[1] * off[1]) + off[2] * off[2]) - sph[3] * sph[3]
        qd = mhb * mhb - qc
        if qd < 0:
            return False, F(0), F(0)
        hs = np.sqrt(qd)
        return True, mhb - hs, mhb + hs


def sphere_test(sph, ray, lo, c):
    """The sphere test with the lower bound lo under the bound c: (accepted, t)."""
    ok, near, far = sphere_roots(sph, ray)
    if not ok:
        return False, F(0)
    if near < c and not (near < lo):
        return True, near
    return bool(far < c and not (far < lo)), far


class RayFilterRef:
    def __init__(self, arrays, masks=None, raw_cache=None):
        """arrays: Scene.arrays() (or OracleScene.arrays()); masks: None or S + T uint32 words; raw_cache: a dict that
        models over the same arrays may share (brute())."""
        self.L = O.lib()
        self.spheres = np.ascontiguousarray(arrays["spheres"], np.float32).reshape(-1, 4)
        self.tris = np.ascontiguousarray(arrays["triangles"], np.float32).reshape(-1, 12)
        self.bvh = np.ascontiguousarray(arrays["bvh"], np.float32).reshape(-1, 8)
        kids = np.ascontiguousarray(self.bvh[:, 6:8]).view(np.int32)
        self.child1 = [int(v) for v in kids[:, 0]]
        self.child2 = [int(v) for v in kids[:, 1]]
        self.S = self.spheres.shape[0]
        self.T = self.tris.shape[0]
        self.masks = None if masks is None else [int(v) for v in np.asarray(masks, np.uint32)]
        self._tri, self._bvh = self.tris.ctypes.data, self.bvh.ctypes.data
        self._tb1, self._tb2 = C.c_float(), C.c_float()
        self._tp1, self._tp2 = C.addressof(self._tb1), C.addressof(self._tb2)
        self._mask_words = None if masks is None else np.asarray(masks, np.uint32).astype(np.uint64)
        self._raw = {} if raw_cache is None else raw_cache     # brute(): ray bytes -> what does not depend on the filter

    # ---- the filter
    def eligible(self, p, skip, rm):
        m = ALL if self.masks is None else self.masks[p]
        return p != skip and (m & rm) != 0

    def _triangle(self, j, o, d, c, lo, skip, rm):
        if not self.L.orc_ray_triangle(self._tri + 48 * j, o, d, float(c), self._tp1):
            return False, F(0)
        t = F(self._tb1.value)
        return (not (t < lo)) and self.eligible(self.S + j, skip, rm), t

    def _sphere(self, k, ray, c, lo, skip, rm):
        ok, t = sphere_test(self.spheres[k], ray, lo, c)
        return ok and self.eligible(k, skip, rm), t

    def _children(self, n, o, d, c):
        """(e1, t1, e2, t2) of node n's children under the bound c."""
        bvh, L = self._bvh, self.L
        c1, c2 = self.child1[n], self.child2[n]
        cf = float(c)
        h1 = bool(L.orc_ray_aabb(bvh + 32 * c1, bvh + 32 * c1 + 12, o, d, cf, self._tp1))
        h2 = bool(L.orc_ray_aabb(bvh + 32 * c2, bvh + 32 * c2 + 12, o, d, cf, self._tp2))
        t1, t2 = F(self._tb1.value), F(self._tb2.value)
        return h1 and not (t1 >= c), t1, h2 and not (t2 >= c), t2

    # ---- the walks
    def closest(self, ray, tmin=None, tmax=None, skip=None, mask=None):
        """-> (t, index, Pn, Iv, Tt, sphere tests, (max depth, overflow pops, discarded pops))."""
        ray = np.ascontiguousarray(ray, np.float32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        lo, closest = lower(tmin), upper(tmax)
        skip = -1 if skip is None else int(skip)
        rm = ALL if mask is None else int(mask)
        index = -1
        pn = iv = tt = st = 0
        depth = opops = disc = 0
        for k in range(self.S):
            st += 1
            ok, t = self._sphere(k, ray, closest, lo, skip, rm)
            if ok:
                closest, index = t, k
        if F(0) >= closest:
            return BIG if index < 0 else closest, index, pn, iv, tt, st, (depth, opops, disc)
        stack = []
        n = 0
        pn += 1
        while True:
            c1, c2 = self.child1[n], self.child2[n]
            descend = False
            if c2 <= c1:
                for j in range(c2, c1):
                    tt += 1
                    ok, t = self._triangle(j, o, d, closest, lo, skip, rm)
                    if ok:
                        closest, index = t, self.S + j
            else:
                iv += 1
                e1, t1, e2, t2 = self._children(n, o, d, closest)
                if e1 or e2:
                    second = e2 and (not e1 or t2 < t1)
                    if e1 and e2:
                        stack.append((c1, t1) if second else (c2, t2))
                        depth = max(depth, len(stack))
                    n = c2 if second else c1
                    pn += 1
                    descend = True
            if descend:
                continue
            found = False
            while stack and not found:
                if len(stack) > CLOSEST_LDS:
                    opops += 1
                node, entry = stack.pop()
                if entry >= closest:
                    disc += 1
                else:
                    n, found = node, True
                    pn += 1
            if not found:
                return BIG if index < 0 else closest, index, pn, iv, tt, st, (depth, opops, disc)

    def anyhit(self, ray, tmin=None, tmax=None, skip=None, mask=None):
        """-> (occluded, Pn, Iv, Tt, sphere tests, (max depth, overflow pops, 0))."""
        ray = np.ascontiguousarray(ray, np.float32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        lo, B = lower(tmin), upper(tmax)
        skip = -1 if skip is None else int(skip)
        rm = ALL if mask is None else int(mask)
        pn = iv = tt = st = 0
        depth = opops = 0
        for k in range(self.S):
            st += 1
            if self._sphere(k, ray, B, lo, skip, rm)[0]:
                return 1, pn, iv, tt, st, (depth, opops, 0)
        if F(0) >= B:
            return 0, pn, iv, tt, st, (depth, opops, 0)
        stack = []
        n = 0
        pn += 1
        while True:
            c1, c2 = self.child1[n], self.child2[n]
            if c2 <= c1:
                for j in range(c2, c1):
                    tt += 1
                    if self._triangle(j, o, d, B, lo, skip, rm)[0]:
                        return 1, pn, iv, tt, st, (depth, opops, 0)
            else:
                iv += 1
                e1, t1, e2, t2 = self._children(n, o, d, B)
                if e1 or e2:
                    second = e2 and (not e1 or t2 < t1)
                    if e1 and e2:
                        stack.append(c1 if second else c2)
                        depth = max(depth, len(stack))
                    n = c2 if second else c1
                    pn += 1
                    continue
            if not stack:
                return 0, pn, iv, tt, st, (depth, opops, 0)
            if len(stack) > ANYHIT_LDS:
                opops += 1
            n = stack.pop()
            pn += 1

    def is_member(self, ray, p, tmin=None, tmax=None, skip=None, mask=None):
        """Whether primitive p is in brute()'s set, and its t there: that primitive's test alone under the bound B."""
        ray = np.ascontiguousarray(ray, np.float32)
        lo, B = lower(tmin), upper(tmax)
        skip = -1 if skip is None else int(skip)
        rm = ALL if mask is None else int(mask)
        if p < self.S:
            return self._sphere(p, ray, B, lo, skip, rm)
        return self._triangle(p - self.S, ray.ctypes.data, ray.ctypes.data + 12, B, lo, skip, rm)

    def brute(self, ray, tmin=None, tmax=None, skip=None, mask=None):
        """Every eligible primitive accepted under the bound B, no tree: [(t, p)]."""
        ray = np.ascontiguousarray(ray, np.float32)
        o, d = ray.ctypes.data, ray.ctypes.data + 12
        lo, B = lower(tmin), upper(tmax)
        skip = -1 if skip is None else int(skip)
        rm = ALL if mask is None else int(mask)
        # What does not depend on the filter is found once per ray: the spheres' roots (sphere_roots, all spheres at
        # once -- numpy rounds each element's operations as the scalar form does), and the triangles accepted under the
        # bound +inf with their t.  The triangle test's last reject is t < kEps or t >= closest and t does not depend on
        # the bound, so the triangles accepted under B <= 1e30 are those with not (t >= B) (a t of +inf fails both).
        key = ray.tobytes()
        raw = self._raw.get(key)
        if raw is None:
            with np.errstate(all="ignore"):
                off = self.spheres[:, :3] - ray[:3]
                dd = ray[3:6]
                mhb = (off[:, 0] * dd[0] + off[:, 1] * dd[1]) + off[:, 2] * dd[2]
                qc = ((off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2]) - self.spheres[:, 3] * self.spheres[:, 3]
                qd = mhb * mhb - qc
                hs = np.sqrt(qd)
                roots = (~(qd < 0), mhb - hs, mhb + hs)
            tt, jj = [], []
            for j in range(self.T):
                if self.L.orc_ray_triangle(self._tri + 48 * j, o, d, float("inf"), self._tp1):
                    tt.append(self._tb1.value)
                    jj.append(self.S + j)
            raw = self._raw[key] = (roots, np.array(tt, np.float32), np.array(jj, np.int64))
        (has, near, far), tt, jj = raw
        with np.errstate(all="ignore"):
            use_near = (near < B) & ~(near < lo)
            ts = np.where(use_near, near, far)
            acc_s = has & (use_near | ((far < B) & ~(far < lo)))
            acc_t = ~(tt >= B) & ~(tt < lo)
        t_all = np.concatenate([ts[acc_s], tt[acc_t]]).astype(np.float32)
        p_all = np.concatenate([np.nonzero(acc_s)[0], jj[acc_t]]).astype(np.int64)
        words = np.full(p_all.shape[0], ALL, np.uint64) if self.masks is None else self._mask_words[p_all]
        keep = (p_all != skip) & ((words & np.uint64(rm)) != 0)
        return [(F(t), int(p)) for t, p in zip(t_all[keep], p_all[keep])]

    # ---- batches: members None or (n,) arrays
    @staticmethod
    def _row(members, i):
        return {k: (None if v is None else v[i]) for k, v in members.items()}

    def closest_batch(self, rays, tmin=None, tmax=None, skip=None, mask=None):
        """-> (t float32 (n,), index int32 (n,), counters int64 (n, 4): Pn Iv Tt sphere tests, life int64 (n, 3))."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        m = dict(tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        t, idx = np.zeros(n, np.float32), np.zeros(n, np.int32)
        ctr, life = np.zeros((n, 4), np.int64), np.zeros((n, 3), np.int64)
        for i in range(n):
            r = self.closest(rays[i], **self._row(m, i))
            t[i], idx[i], ctr[i], life[i] = r[0], r[1], r[2:6], r[6]
        return t, idx, ctr, life

    def anyhit_batch(self, rays, tmin=None, tmax=None, skip=None, mask=None):
        """-> (occluded bool (n,), counters int64 (n, 4), life int64 (n, 3))."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        m = dict(tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        occ = np.zeros(n, np.bool_)
        ctr, life = np.zeros((n, 4), np.int64), np.zeros((n, 3), np.int64)
        for i in range(n):
            r = self.anyhit(rays[i], **self._row(m, i))
            occ[i], ctr[i], life[i] = bool(r[0]), r[1:5], r[5]
        return occ, ctr, life

    def brute_batch(self, rays, tmin=None, tmax=None, skip=None, mask=None):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        m = dict(tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        return [self.brute(rays[i], **self._row(m, i)) for i in range(rays.shape[0])]
