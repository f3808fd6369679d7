"""Synthetic scene files that drive traversal paths the shipped scenes reach rarely or never.

* big_leaf: 80 triangles with one common centroid (rotated copies).  The binned SAH split
  (scene.cu:866-1000) finds min_centroid == max_centroid on every axis, so they end in one leaf
  of 80 triangles: the renderer's leaf refs hold at most 63 inline, larger leaves go through the
  indirection table.
* deep: 60 triangles at x = 3^k.  The binned split peels off the farthest triangle at every
  level, so the tree is a chain as deep as MAX_BVH_DEPTH (30, scene.cu:10) allows.  A ray
  coming from +x enters each level's single-triangle child first, so the reference pushes that
  near child and descends into the far subtree: the stack grows by one per level, past the
  8 entries the trace kernel keeps in LDS into its global overflow.  The triangles' yz
  projections box the x axis without covering it, so rays along the axis hit nothing and walk
  the whole chain.
"""
import math
import os

import numpy as np


def _tri(p, q, r):
    return "triangle white %s %s %s\n" % tuple(" ".join("%.9g" % c for c in v) for v in (p, q, r))


DEEP_COUNT, DEEP_RATIO = 60, 3.0   # a 30-level chain (59 nodes): one triangle split off per level

HEADER = ("material white diffuse 0.8 0.8 0.8 metallicity 0.2 specular 1 1 1 roughness 0.3\n"
          "material grey diffuse 0.5 0.5 0.5\n"
          "sky 0.6 0.7 0.9\n")


def big_leaf_scene():
    s = HEADER
    for k in range(80):
        a = 2 * math.pi * k / 80
        dx, dz = 0.5 * math.cos(a), 0.5 * math.sin(a)
        # p and q mirror each other about the y axis (their printed x and z negate exactly) and
        # r = (0, 0, 0): the float centroid of every triangle is exactly (0, 1, 0)
        s += _tri((dx, 1.5, dz), (-dx, 1.5, -dz), (0.0, 0.0, 0.0))
    s += "quad grey -20 0 -20 -20 0 20 20 0 20 20 0 -20\n"
    s += "camera position -4 1.5 0 forward 1 -0.1 0 up 0 1 0 fov 40\n"
    s += "image 48 32 20 4 1\n"
    return s


def deep_scene():
    s = HEADER
    for k in range(DEEP_COUNT):
        x = DEEP_RATIO ** k
        # yz projection (-1, 1.2), (1, 1), (1.2, -1): its box holds (0, 0), the triangle does not
        s += _tri((x, -1.0, 1.2), (x + 0.01, 1.0, 1.0), (x + 0.02, 1.2, -1.0))
    s += "camera position 1e29 0.05 0.05 forward -1 0 0 up 0 1 0 fov 2\n"
    s += "image 32 32 20 3 1\n"
    return s


# ---------------------------------------------------------------- ray sets for deep.scene
# Every triangle of deep has the yz projection (-1, 1.2), (1, 1), (1.2, -1): (0.4, 0.4) lies inside it, the
# x axis runs through the gap it leaves.  The *_plus sets run toward +x, the direction in which the any-hit
# kernel (near child first, far child pushed) stacks one entry per level; the *_minus sets run toward -x,
# the direction in which the reference's order (trace_kernel) does.  All are seeded: the same (n, seed)
# gives the same floats.

def _unit(v):
    v = np.asarray(v, np.float32)
    return (v / np.sqrt((v * v).sum(-1, keepdims=True)).astype(np.float32)).astype(np.float32)


def _gap_yz(n, rng):
    return (rng.random((n, 2)) * 0.2 - 0.1).astype(np.float32)       # inside every triangle's gap


def _rays(o, d):
    return np.ascontiguousarray(np.hstack([o, d]), np.float32)


def axis_plus(n, seed=21):
    """From x = -5 along +x through the gap: the whole chain is walked, nothing is hit."""
    rng = np.random.default_rng(seed)
    o = np.hstack([np.full((n, 1), -5.0, np.float32), _gap_yz(n, rng)])
    return _rays(o, np.tile(np.array([[1, 0, 0]], np.float32), (n, 1)))


def solid_plus(n, seed=21):
    """axis_plus shifted by +0.5 in y and z, into the triangles: stopped by triangle 0, which the any-hit
    kernel reaches in the bottom leaf with one pushed node per level above it still on the stack."""
    r = axis_plus(n, seed)
    r[:, 1:3] += np.float32(0.5)
    return r


def tilted_plus(n, seed=22):
    """From (0.5, y, z) in the gap along normalize(1, 1.3 * 3^-k, 0), k uniform in [5, 59): the ray leaves the
    triangles' common yz box near x = 3^k, so only the levels below that point push, and it is stopped on the
    way out (where y is in 0.2 .. 1.1 at a triangle's x), after pops."""
    rng = np.random.default_rng(seed)
    o = np.hstack([np.full((n, 1), 0.5, np.float32), _gap_yz(n, rng)])
    k = 5 + 54 * rng.random(n)
    d = np.stack([np.ones(n), 1.3 * DEEP_RATIO ** -k, np.zeros(n)], 1)
    return _rays(o, _unit(d))


def _start_x(n, rng):
    # between triangles j and j + 1, j uniform in 30 .. 59: the triangles past the origin are behind the ray,
    # so rays differ in the level at which they start to push (j < 31 starts inside the bottom leaf's box)
    return (2.0 * DEEP_RATIO ** rng.integers(30, DEEP_COUNT, n)).astype(np.float32).reshape(n, 1)


def axis_minus(n, seed=23):
    """Along -x through the gap, from between two triangles of the chain: nothing is hit."""
    rng = np.random.default_rng(seed)
    yz = _gap_yz(n, rng)
    return _rays(np.hstack([_start_x(n, rng), yz]), np.tile(np.array([[-1, 0, 0]], np.float32), (n, 1)))


def solid_minus(n, seed=23):
    """axis_minus shifted by +0.5 in y and z: the closest hit is the first triangle below the origin's x, found
    after the reference's order has walked to the bottom of the chain and back."""
    r = axis_minus(n, seed)
    r[:, 1:3] += np.float32(0.5)
    return r


def tilted_minus(n, seed=24):
    """tilted_plus's lines walked the other way: from x = 0.5 + 4 * 3^k, outside the common yz box, toward
    (0.5, y, z) in the gap; the ray enters the box near x = 3^k and meets a triangle soon after."""
    rng = np.random.default_rng(seed)
    p = np.hstack([np.full((n, 1), 0.5, np.float32), _gap_yz(n, rng)]).astype(np.float64)
    k = 5 + 54 * rng.random(n)
    u = np.stack([np.ones(n), 1.3 * DEEP_RATIO ** -k, np.zeros(n)], 1)
    o = p + (4.0 * DEEP_RATIO ** k)[:, None] * u
    return _rays(o.astype(np.float32), _unit(-u))


def interleaved(*sets):
    """Ray i of each set in turn: with three sets every 64-lane wave holds rays of all three."""
    n = min(s.shape[0] for s in sets)
    return np.ascontiguousarray(np.stack([s[:n] for s in sets], 1).reshape(-1, 6), np.float32)


def write(dirpath):
    """Writes big_leaf.scene and deep.scene into dirpath; returns their paths."""
    out = {}
    for name, text in (("big_leaf", big_leaf_scene()), ("deep", deep_scene())):
        p = os.path.join(dirpath, name + ".scene")
        with open(p, "w") as f:
            f.write(text)
        out[name] = p
    return out
