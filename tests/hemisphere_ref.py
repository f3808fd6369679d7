"""Yardstick of the hemisphere visibility queries (rt_abi.h) -- TEST INFRASTRUCTURE ONLY.

The sample generator restated in numpy with no call into the product's library: PCG in uint64 / uint32 arithmetic,
random_radians in float64, everything else float32 with each operation rounded once, in the order rt_abi.h states:

  nh  = (1 / sqrt((x x + y y) + z z)) * nrm
  w   = (point_offset + i) * S + s                                   (uint32, wraps)
  rng = pcg_seed(w * 0x9E3779B1 + seed * 0x85EBCA6B);  u = random_on_sphere(rng)
  cosine   v = nh + u, m = magsq(v), dir = nh if not (m >= 2^-40) else (1 / sqrt(m)) * v
  uniform  dir = -u if dot(u, nh) < 0 else u

random_on_sphere here (two PCG draws, the Cody-Waite sin/cos, sqrt) is checked against the oracle's
orc_random_on_sphere(seed, 1, .) on every work item that is generated: a difference raises.
Occlusion is RayFilterRef.anyhit's (tests/ray_filter_ref.py), the pinned filtered any-hit walk with its counters.
"""
import ctypes as C

import numpy as np

import oracle_lib as O
from ray_filter_ref import RayFilterRef

F = np.float32
U32, U64 = np.uint32, np.uint64
MODES = {"cosine": 0, "uniform": 1}
PCG_MUL = U64(6364136223846793005)
SEED_MUL = U64(6839056345687307)
PCG_INC = U64(820957824423429)
TINY = F(2.0 ** -40)


def _pcg(state):
    """One PCG-XSH-RR step over a uint64 array: (next state, uint32 output)."""
    old = state
    with np.errstate(over="ignore"):
        nxt = old * PCG_MUL + (PCG_INC | U64(1))
    xs = (((old >> U64(18)) ^ old) >> U64(27)).astype(U32)
    rot = (old >> U64(59)).astype(U32)
    with np.errstate(over="ignore"):
        back = (U32(0) - rot) & U32(31)
    return nxt, (xs >> rot) | (xs << back)


def _sincos(x):
    """rt_sincos restated: Cody-Waite reduction by pi/2 and the cephes polynomials, float32, fixed order, x >= 0."""
    x = x.astype(F)
    fj = x * F(0.636619772)
    j = (fj + F(0.5)).astype(np.int32)
    jf = j.astype(F)
    r = ((x - jf * F(1.5703125)) - jf * F(4.837512969970703125e-4)) - jf * F(7.54978995489188216e-8)
    z = r * r
    sp = ((F(-1.9515295891e-4) * z + F(8.3321608736e-3)) * z - F(1.6666654611e-1)) * z * r + r
    cp = ((F(2.443315711809948e-5) * z - F(1.388731625493765e-3)) * z + F(4.166664568298827e-2)) * z * z - F(0.5) * z + F(1.0)
    q = j & 3
    odd = (q & 1) != 0
    a, b = np.where(odd, cp, sp), np.where(odd, sp, cp)
    return np.where((q & 2) != 0, -a, a).astype(F), np.where(((q + 1) & 2) != 0, -b, b).astype(F)


def sphere_samples(seeds, check=True):
    """random_on_sphere(pcg_seed(seed)) for a uint32 array of seeds: (k, 3) float32, checked against the oracle."""
    seeds = np.asarray(seeds, U32)
    with np.errstate(over="ignore"):
        st = seeds.astype(U64) * SEED_MUL
    st, _ = _pcg(st)
    st, a = _pcg(st)
    st, b = _pcg(st)
    r1 = (a.astype(np.float64) * (3.14159265358979323846 * 2 / 4294967295.0)).astype(F)
    r2 = b.astype(F) * F(2.0 ** -31)
    x = np.sqrt(r2 * (F(2) - r2))
    s, c = _sincos(r1)
    u = np.stack([c * x, s * x, F(1) - r2], 1).astype(F)
    if check:
        L = O.lib()
        buf = np.zeros(3, F)
        p = buf.ctypes.data_as(C.c_void_p)
        for k in range(seeds.shape[0]):
            L.orc_random_on_sphere(int(seeds[k]), 1, p)
            if buf.tobytes() != u[k].tobytes():
                raise AssertionError("yardstick random_on_sphere differs from the oracle at seed %d: %r vs %r" % (seeds[k], u[k], buf))
    return u


def _magsq(v):
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def unit_normals(normals):
    nm = np.ascontiguousarray(normals, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt(_magsq(nm))
        return (inv[:, None] * nm).astype(F)


def work_items(n, samples, point_offset, first=None):
    """(point index i, uint32 w) of the first `first` (None: all n * samples) work items in the order i * S + s."""
    total = n * samples if first is None else min(first, n * samples)
    k = np.arange(total, dtype=np.int64)
    i, s = k // samples, k % samples
    w = (((int(point_offset) + i) * samples + s) & 0xFFFFFFFF).astype(U32)
    return i, w


def rays(points, normals, samples, mode="cosine", seed=0, point_offset=0, first=None, check=True):
    """The sample rays (m, 6) float32 of the first `first` work items (None: all)."""
    pts = np.ascontiguousarray(points, F).reshape(-1, 3)
    nh_all = unit_normals(normals)
    i, w = work_items(pts.shape[0], int(samples), point_offset, first)
    with np.errstate(over="ignore"):
        seeds = w * U32(0x9E3779B1) + U32((int(seed) * 0x85EBCA6B) & 0xFFFFFFFF)
    u = sphere_samples(seeds, check)
    nh = nh_all[i]
    with np.errstate(all="ignore"):
        if MODES[mode] == 1:
            dot = (u[:, 0] * nh[:, 0] + u[:, 1] * nh[:, 1]) + u[:, 2] * nh[:, 2]
            d = np.where((dot < 0)[:, None], -u, u)
        else:
            v = nh + u
            m = _magsq(v)
            inv = F(1) / np.sqrt(m)
            d = np.where((~(m >= TINY))[:, None], nh, inv[:, None] * v)
    return np.ascontiguousarray(np.hstack([pts[i], d.astype(F)]), F)


class HemisphereRef:
    def __init__(self, arrays, masks=None):
        self.walk = RayFilterRef(arrays, masks)

    def run(self, points, normals, samples, mode="cosine", seed=0, point_offset=0, tmin=None, tmax=None, skip=None, mask=None,
            first=None):
        """Over the first `first` work items (None: all): dict(open_count int64 (n,) -- the escaped rays among the
        walked ones of each point --, walked int64 (n,), counters int64 (4,): Pn Iv Tt sphere tests summed, depth: the
        deepest stack after a push, overflow_pops: pops from entries past the kernel's LDS entries, rays)."""
        pts = np.ascontiguousarray(points, F).reshape(-1, 3)
        n = pts.shape[0]
        r = rays(pts, normals, samples, mode, seed, point_offset, first)
        idx, _ = work_items(n, int(samples), point_offset, first)
        open_count, walked = np.zeros(n, np.int64), np.zeros(n, np.int64)
        ctr = np.zeros(4, np.int64)
        depth = opops = 0
        row = lambda a, i: None if a is None else a[i]
        for k in range(r.shape[0]):
            i = int(idx[k])
            res = self.walk.anyhit(r[k], row(tmin, i), row(tmax, i), row(skip, i), row(mask, i))
            open_count[i] += 0 if res[0] else 1
            walked[i] += 1
            ctr += np.array(res[1:5], np.int64)
            depth, opops = max(depth, res[5][0]), opops + res[5][1]
        return dict(open_count=open_count, walked=walked, counters=ctr, depth=depth, overflow_pops=opops, rays=r)
