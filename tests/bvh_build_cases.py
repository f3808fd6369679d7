"""Seeded scene texts that aim the BVH build (host/scene_load.cpp, csrc/bvh_build.hip) at the places
where the device build changes its code path.  cases() maps a name to a scene text; tests/bvh_build_ref.py
certifies (tests/test_bvh_build_cases.py::test_cases_reach_their_paths) that each family reaches the path
it is named for.

The device build has three launch regimes by node length: at most 4096 triangles (one wave, tiles of
256), 4097..32768 (1024 lanes, tiles of 4096), and above 32768 (chunks of 8192, one workgroup each).

* size_N / sorted_N: one soup of 40,961 triangles (half of them on a lattice of ties and signed zeros,
  every tenth an exact duplicate of the one before it) cut to its first N triangles; N sits on every
  regime and tile edge (4096/4097, 32768/32769, 256/257, 8192/8193), on a last chunk of one triangle
  (32769, 40961) and on an exact chunk multiple (40960).  sorted_N is the same cut ordered by descending
  centroid along the axis its root splits on (the soup's outliers move that axis from cut to cut, so
  ordering by x alone would leave most roots unsorted along their own axis): at the root every element
  starts on the wrong side of the split.
* line_N: centroids vary along x only; y and z have min_centroid == max_centroid and are skipped.
* same_centroid_N: rotated copies about one centroid, some of them exact duplicates: no axis to split on,
  the root is a leaf of N.
* chain_N: a cluster of N small triangles in the unit cube and 30 outliers at x = 9^k.  Every level's bins
  hold the farthest outlier in the last bin and everything else in the first, so each level peels off one
  outlier and the cluster arrives at depth 30 (MAX_BVH_DEPTH) as one leaf: a node that may not split.
  (With a ratio of 8 the second outlier sits on the edge between the first two bins; 9 keeps it inside
  the first.)
* adjacent_floats_N: centroid x is 1e8 for one group (small boxes) and a few floats above it for the
  other (large boxes).  The bins separate the groups and the split is cheaper than the node, but the split
  position min_centroid + step * 1 rounds back to 1e8, so nobody is left of it: a degenerate partition
  (L == 0) that permutes the range and leaves the node a leaf.
* denormal_range_N: centroid x is 0 for one group and 16 or 24 denormal steps (of 2^-149) for the other, so
  the range is below 8 / FLT_MAX and the bin scale 8 / range is infinite: the scaled offset is NaN at the
  minimum and inf above it.  The reference's conversion of those to a bin index is undefined; host build,
  oracle and device build all define it as NaN -> bin 0, inf -> the last bin.  The split position
  0 + (24 steps / 8) * 1 is exact, so the partition is a real one: the first group goes left.
* points_on_line: 200 point-sized triangles on a line parallel to x: every box area, so every cost, is 0.
* mixed_level: clusters of 32,769, 49,153 and 5,000 triangles and 40 stragglers, shuffled.  The root
  separates {cluster 1, stragglers} from {cluster 2, cluster 3}; the next level separates each pair, so
  depth 2 holds two chunked nodes of 5 and 7 chunks, a 1024-lane node and a one-wave node.

Every coordinate is a float32 written with repr(float(x)), so the text parses back to exactly that float.
Materials are assigned i % 5 by input index: exact duplicates sit next to each other and so differ in
material.
"""
import collections.abc
import math

import numpy as np

import bvh_build_ref
import edge_scenes

MATERIALS = ("white", "grey", "red", "green", "blue")
HEADER = (edge_scenes.HEADER.replace("sky", "material red diffuse 0.8 0.1 0.1\n"
                                            "material green diffuse 0.1 0.8 0.1 metallicity 1 roughness 0.1\n"
                                            "material blue diffuse 0.1 0.1 0.8\nsky", 1))
FOOTER = "camera position 0 0 -10 forward 0 0 1 up 0 1 0 fov 40\nimage 16 16 1 1 1\n"

SIZES = (1, 4, 5, 63, 64, 65, 256, 257, 4095, 4096, 4097, 8192, 8193, 32767, 32768, 32769, 40960, 40961)
SOUP_MAX = 40961
LINE = SAME_CENTROID = (4097, 32769)
CHAIN = (5000, 33000)
CHAIN_OUTLIERS, CHAIN_RATIO = 30, 9.0
ADJACENT = DENORMAL = (6, 5000, 33000)
MIXED = (32769, 49153, 5000, 40)      # three clusters and the stragglers


def triangle_lines(verts, first_material=0):
    """verts (n, 9) float32 -> one `triangle` line each, material (first_material + i) % 5."""
    verts = np.asarray(verts, np.float32).reshape(-1, 9)
    return ["triangle %s %s\n" % (MATERIALS[(first_material + i) % 5], " ".join(repr(float(x)) for x in v))
            for i, v in enumerate(verts)]


def scene_text(lines):
    return HEADER + "".join(lines) + FOOTER


def centroids(verts):
    """The loader's centroid: (1/3f) * ((p1 + p2) + p3) in float32."""
    v = np.asarray(verts, np.float32).reshape(-1, 3, 3)
    return (np.float32(1.0) / np.float32(3.0)) * ((v[:, 0] + v[:, 1]) + v[:, 2])


def soup_vertices(n=SOUP_MAX, seed=11):
    rng = np.random.default_rng(seed)
    vals = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0], np.float32)
    ties = rng.choice(vals, size=(n, 9))                                   # ties and signed zeros
    free = (rng.normal(size=(n, 9)) * rng.choice([0.01, 1.0, 100.0], size=(n, 1))).astype(np.float32)
    v = np.where(rng.random((n, 1)) < 0.5, ties, free).astype(np.float32)
    v[9::10] = v[8::10][:v[9::10].shape[0]]                               # exact duplicates, adjacent
    return v


def sorted_by_root_axis(verts):
    """Descending centroid order along the axis the root splits on (x where it does not split).  The
    soup's outliers make that axis vary with the cut; ordering by x alone would leave most cuts unsorted
    along the axis that their root partitions."""
    axis = max(0, bvh_build_ref.decide(*bvh_build_ref.build_input(verts), bvh_build_ref.MAX_DEPTH).axis)
    return verts[np.argsort(-centroids(verts)[:, axis], kind="stable")]


def line_vertices(n, seed=12):
    """Triangles in planes x = const: p1 = (x, -a, -b), p2 = (x, 0, b), p3 = (x, a, 0), so the float
    centroid's y and z are exactly 0; x is a multiple of 1/64 in [0, 100), with many ties."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 6400, n) / 64.0).astype(np.float32)
    a = (0.1 + rng.random(n)).astype(np.float32)
    b = (0.1 + rng.random(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    return np.stack([x, -a, -b, x, z, b, x, a, z], 1)


def same_centroid_vertices(n):
    """edge_scenes.big_leaf_scene's rotated copies: (dx, 1.5, dz), (-dx, 1.5, -dz), (0, 0, 0); every
    seventh triangle repeats the one before it exactly."""
    k = np.arange(n)
    ang = 2 * math.pi * k / n
    dx, dz = (0.5 * np.cos(ang)).astype(np.float32), (0.5 * np.sin(ang)).astype(np.float32)
    h, z = np.full(n, 1.5, np.float32), np.zeros(n, np.float32)
    v = np.stack([dx, h, dz, -dx, h, -dz, z, z, z], 1)
    v[6::7] = v[5::7][:v[6::7].shape[0]]
    return v


def small_triangles(n, rng, lo, hi, size=0.01, grid=1024.0):
    """n triangles of extent ~size with one corner uniform in the box [lo, hi], on a grid of 1/grid."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = np.round((lo + rng.random((n, 3)) * (hi - lo - size)) * grid) / grid
    e = np.round(rng.random((n, 2, 3)) * size * grid + 1.0) / grid
    return np.concatenate([p, p + e[:, 0], p + e[:, 1]], 1).astype(np.float32)


def chain_vertices(n, seed=13):
    rng = np.random.default_rng(seed + n)
    cluster = small_triangles(n, rng, (0, 0, 0), (1, 1, 1))
    out = np.zeros((CHAIN_OUTLIERS, 9), np.float32)
    for k in range(1, CHAIN_OUTLIERS + 1):
        x = CHAIN_RATIO ** k
        out[k - 1] = [x, 0.5, 0.5, x, 0.51, 0.5, x, 0.5, 0.51]
    v = np.concatenate([cluster, out])
    return v[rng.permutation(v.shape[0])]


def adjacent_float_vertices(n, seed=14):
    """All three vertices of a triangle share x = 1e8 + 8 j (8 is the float spacing there): j = 0 for the
    first group, whose float centroid x is exactly 1e8, j in 1..4 for the second (centroids 16, 24 or 32
    above).  y and z are (-a, 0, a) and (-b, b, 0): their centroids are exactly 0, the boxes have area;
    the first group's a, b are ten times smaller, so splitting the groups apart is cheaper than the node."""
    rng = np.random.default_rng(seed + n)
    second = np.arange(n) % 2 == 1
    j = np.where(second, 1 + np.arange(n) // 2 % 4, 0)
    x = (np.float32(1e8) + np.float32(8.0) * j.astype(np.float32)).astype(np.float32)
    a = ((0.1 + rng.random(n)) * np.where(second, 5.0, 0.5)).astype(np.float32)
    b = ((0.1 + rng.random(n)) * np.where(second, 5.0, 0.5)).astype(np.float32)
    z = np.zeros(n, np.float32)
    return np.stack([x, -a, -b, x, z, b, x, a, z], 1)


def denormal_range_vertices(n, seed=17):
    """adjacent_float_vertices with x = 0 for the first group and 16 or 24 times 2^-149 for the second."""
    rng = np.random.default_rng(seed + n)
    second = np.arange(n) % 2 == 1
    steps = np.where(second, 16 + 8 * (np.arange(n) // 2 % 2), 0).astype(np.int32)
    x = steps.view(np.float32)                     # a denormal's bits are its count of 2^-149 steps
    a = ((0.1 + rng.random(n)) * np.where(second, 5.0, 0.5)).astype(np.float32)
    b = ((0.1 + rng.random(n)) * np.where(second, 5.0, 0.5)).astype(np.float32)
    z = np.zeros(n, np.float32)
    return np.stack([x, -a, -b, x, z, b, x, a, z], 1)


def points_on_line_vertices(n=200, seed=15):
    rng = np.random.default_rng(seed)
    x = (rng.integers(-500, 500, n) / 8.0).astype(np.float32)
    p = np.stack([x, np.full(n, 1.0, np.float32), np.full(n, 2.0, np.float32)], 1)
    return np.concatenate([p, p, p], 1)


def mixed_level_vertices(seed=16):
    rng = np.random.default_rng(seed)
    n1, n2, n3, ns = MIXED
    v = np.concatenate([small_triangles(n1, rng, (0, 0, 0), (1, 1, 1)),
                        small_triangles(ns, rng, (6, 0, 0), (6.2, 1, 1)),
                        small_triangles(n2, rng, (20, 0, 0), (21, 1, 1)),
                        small_triangles(n3, rng, (27, 0, 0), (28, 1, 1))])
    return v[rng.permutation(v.shape[0])]


def names():
    out = ["size_%d" % n for n in SIZES] + ["sorted_%d" % n for n in SIZES]
    out += ["line_%d" % n for n in LINE] + ["same_centroid_%d" % n for n in SAME_CENTROID]
    out += ["chain_%d" % n for n in CHAIN] + ["adjacent_floats_%d" % n for n in ADJACENT]
    out += ["denormal_range_%d" % n for n in DENORMAL]
    return out + ["points_on_line", "mixed_level"]


_verts = {}


def vertices(name):
    """The case's input triangles, (n, 9) float32 in input order (material i % 5)."""
    if name not in _verts:
        family, _, arg = name.rpartition("_")
        if name in ("points_on_line", "mixed_level"):
            v = points_on_line_vertices() if name == "points_on_line" else mixed_level_vertices()
        elif family in ("size", "sorted"):
            if "soup" not in _verts:
                _verts["soup"] = soup_vertices()
            v = _verts["soup"][:int(arg)]
            v = sorted_by_root_axis(v) if family == "sorted" else v
        else:
            v = {"line": line_vertices, "same_centroid": same_centroid_vertices, "chain": chain_vertices,
                 "adjacent_floats": adjacent_float_vertices, "denormal_range": denormal_range_vertices}[family](int(arg))
        _verts[name] = v
    return _verts[name]


def materials(name):
    return (np.arange(vertices(name).shape[0]) % 5).astype(np.uint16)


_soup_lines = {}


def text(name):
    family, _, arg = name.rpartition("_")
    if family == "size":              # the cuts share the soup's lines
        if not _soup_lines:
            _soup_lines[0] = triangle_lines(vertices("size_%d" % SOUP_MAX))
        return scene_text(_soup_lines[0][:int(arg)])
    return scene_text(triangle_lines(vertices(name)))


class _Cases(collections.abc.Mapping):
    """{name: text}; a text is made when it is asked for (together they are some hundred megabytes)."""

    def __getitem__(self, name):
        if name not in names():
            raise KeyError(name)
        return text(name)

    def __iter__(self):
        return iter(names())

    def __len__(self):
        return len(names())


def cases():
    return _Cases()


def write(name, dirpath):
    p = "%s/%s.scene" % (dirpath, name)
    with open(p, "w") as f:
        f.write(text(name))
    return p
