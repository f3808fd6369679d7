"""The host BVH build (host/scene_load.cpp) on the inputs of tests/bvh_build_cases.py, against two
yardsticks: the numpy model of the reference's node decision (tests/bvh_build_ref.py) and the oracle's
restated loader.  The model also certifies that every case reaches the path of the build it is named
for (test_cases_reach_their_paths): those assertions are conditions on the inputs.  The device build is
compared with the host build on the same cases in tests/test_gpu_bvh_build.py.  No GPU here."""
import numpy as np
import pytest

import bvh_build_cases as cases
import bvh_build_ref as ref
import oracle_lib as O
import rtamd as R

NAMES = cases.names()
FULL_MODEL_MAX = 8193          # larger cases are compared at the root only
HUGE, BIG_MIN, CHUNK = 32768, 4096, 8192     # csrc/bvh_build.hip: kHuge, kBigMin, kChunk


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("bvh_build_cases"))


_paths, _host, _model, _root = {}, {}, {}, {}


def path_of(name, scene_dir):
    if name not in _paths:
        _paths[name] = cases.write(name, scene_dir)
    return _paths[name]


def host_arrays(name, scene_dir):
    if name not in _host:
        _host[name] = R.Scene(path_of(name, scene_dir)).arrays()
    return _host[name]


def model(name):
    if name not in _model:
        _model[name] = ref.build(cases.vertices(name), cases.materials(name))
    return _model[name]


def root_decision(name):
    if name in _model:
        return _model[name][0][0].decision
    if name not in _root:
        blo, bhi, cen = ref.build_input(cases.vertices(name))
        _root[name] = ref.decide(blo, bhi, cen, ref.MAX_DEPTH)
    return _root[name]


def rows(tri9, mats):
    """(n, 9) float32 and (n,) uint16 -> one sortable byte string per triangle."""
    return [a.tobytes() + b.tobytes() for a, b in zip(np.ascontiguousarray(tri9, np.float32), np.asarray(mats, np.uint16))]


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_model(name, scene_dir):
    """Node array, triangle order and material order of the host build equal the model's recursion; for
    cases above 8,193 triangles, the root's box, its split index and the contents of its two ranges."""
    h = host_arrays(name, scene_dir)
    verts, mats = cases.vertices(name), cases.materials(name)
    tri9 = ref.render_triangles(verts)
    assert h["triangles"].shape[0] == verts.shape[0]
    if verts.shape[0] <= FULL_MODEL_MAX:
        nodes, perm = model(name)
        assert h["bvh"].tobytes() == ref.node_array(nodes).tobytes()
        assert h["triangles"][:, 0:9].tobytes() == tri9[perm].tobytes()
        assert h["material_indices"].tobytes() == mats[perm].tobytes()
        return
    d = root_decision(name)
    assert h["bvh"][0, 0:3].tobytes() == d.lo.tobytes() and h["bvh"][0, 3:6].tobytes() == d.hi.tobytes()
    _, length, leaf = ref.walk(h["bvh"])
    order = np.asarray(d.order)
    got, want = rows(h["triangles"][:, 0:9], h["material_indices"]), rows(tri9[order], mats[order])
    if d.axis < 0 or d.degenerate:
        assert leaf[0] and h["bvh"].shape[0] == 1
        assert got == want                                  # one leaf: the root's own (permuted) order
        return
    kids = np.ascontiguousarray(h["bvh"][0, 6:8]).view(np.int32)
    assert not leaf[0] and length[kids[0]] == d.L and length[kids[1]] == d.count - d.L
    assert sorted(got[:d.L]) == sorted(want[:d.L]) and sorted(got[d.L:]) == sorted(want[d.L:])


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_oracle(name, scene_dir):
    a = O.OracleScene(path_of(name, scene_dir)).arrays()
    b = host_arrays(name, scene_dir)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["size_32769", "chain_33000", "mixed_level"])
def test_host_build_independent_of_threads(name, scene_dir, monkeypatch):
    out = {}
    for threads in ("1", "16"):
        monkeypatch.setenv("RT_BVH_THREADS", threads)
        out[threads] = R.Scene(path_of(name, scene_dir)).arrays()
    for k in ("bvh", "triangles", "material_indices"):
        assert out["1"][k].tobytes() == out["16"][k].tobytes(), k


def chunks_of(length):
    return -(-int(length) // CHUNK)


def test_cases_reach_their_paths(scene_dir):
    """Conditions on the inputs: each family reaches the path of csrc/bvh_build.hip it is named for."""
    for n in cases.CHAIN:                      # a leaf of n or more at depth 30 that may not split; 61 nodes
        bvh = host_arrays("chain_%d" % n, scene_dir)["bvh"]
        depth, length, leaf = ref.walk(bvh)
        assert bvh.shape[0] == 2 * cases.CHAIN_OUTLIERS + 1 == 61
        assert depth.max() == ref.MAX_DEPTH
        assert any(leaf[x] and depth[x] == ref.MAX_DEPTH and length[x] >= n for x in range(61)), n
    for name in ["same_centroid_%d" % n for n in cases.SAME_CENTROID] + ["points_on_line"]:
        assert host_arrays(name, scene_dir)["bvh"].shape[0] == 1, name
        d = root_decision(name)
        assert d.may_split and d.axis < 0
        if name == "points_on_line":           # every cost is 0, the node's own included
            assert d.skipped == [False, True, True] and d.zero_costs == 7 and d.own_cost == 0
        else:
            assert d.skipped == [True, True, True]
    for n in cases.LINE:
        d = root_decision("line_%d" % n)
        assert d.skipped == [False, True, True] and d.axis == 0 and not d.degenerate
    for n in cases.ADJACENT:                   # a split cheaper than the node that leaves nobody on the left
        d = root_decision("adjacent_floats_%d" % n)
        assert d.axis == 0 and d.best_cost < d.own_cost and d.degenerate and d.L == 0
        assert d.pos == np.float32(1e8) and d.order != list(range(n))
        assert host_arrays("adjacent_floats_%d" % n, scene_dir)["bvh"].shape[0] == 1
    for n in cases.DENORMAL:                   # an infinite bin scale: NaN and inf offsets, and a real split
        d = root_decision("denormal_range_%d" % n)
        assert d.inf_scale == [True, False, False] and d.skipped == [False, True, True]
        assert d.axis == 0 and not d.degenerate and d.L == (n + 1) // 2 and 0 < d.pos < 1e-44
        assert host_arrays("denormal_range_%d" % n, scene_dir)["bvh"].shape[0] >= 3
    for n in cases.SIZES[2:]:                  # the sorted soup: everybody starts on the wrong side of the root
        d = root_decision("sorted_%d" % n)
        cen = ref.build_input(cases.vertices("sorted_%d" % n))[2][:, d.axis]
        assert d.axis >= 0 and 0 < d.L < n
        assert not (cen[:n - d.L] < d.pos).any() and (cen[n - d.L:] < d.pos).all()
    depth, length, _ = ref.walk(host_arrays("mixed_level", scene_dir)["bvh"])
    found = False
    for lv in range(int(depth.max()) + 1):
        lens = length[depth == lv]
        huge_chunks = {chunks_of(x) for x in lens if x > HUGE}
        found |= (len(huge_chunks) >= 2 and ((lens > BIG_MIN) & (lens <= HUGE)).any() and (lens <= BIG_MIN).any())
    assert found
    lens2 = sorted(length[depth == 2])         # as designed: stragglers, cluster 3, cluster 1 (5 chunks), cluster 2 (7)
    assert lens2 == sorted(cases.MIXED) and chunks_of(lens2[2]) == 5 and chunks_of(lens2[3]) == 7


def test_degenerate_partition_with_everybody_left_is_not_found():
    """L == n (everybody left of the split) needs position > max_centroid.  The position is
    min_centroid + step * (i + 1) with i + 1 <= 7 and step = (max_centroid - min_centroid) / 8, every
    operation rounded to nearest and so monotone: it cannot pass max_centroid, whose own element is then
    not left of it.  A seeded search agrees: 3,000 node decisions over adjacent-float centroid sets
    (6..40 triangles, centroids within a few floats of a random magnitude, box sizes per group random)
    give 0 cases of L == n (and hundreds of L == 0).  So there is no such case in bvh_build_cases."""
    rng = np.random.default_rng(2024)
    tried = zero = full = 0
    for _ in range(3000):
        n = int(rng.integers(6, 41))
        base = np.float32(rng.choice([1.0, -1.0]) * 10.0 ** rng.uniform(-3, 9))
        up = np.float32(np.inf if rng.random() < 0.5 else -np.inf)
        ladder = [base]
        for _ in range(int(rng.integers(1, 6))):
            ladder.append(np.nextafter(ladder[-1], up))
        cx = np.array(ladder, np.float32)[rng.integers(0, len(ladder), n)]
        ext = (rng.random((n, 2)) * np.where(cx == base, 0.5, 5.0)[:, None]).astype(np.float32)
        cen = np.stack([cx, np.zeros(n, np.float32), np.zeros(n, np.float32)], 1)
        blo = np.stack([cx, -ext[:, 0], -ext[:, 1]], 1)
        bhi = np.stack([cx, ext[:, 0], ext[:, 1]], 1)
        d = ref.decide(blo, bhi, cen, ref.MAX_DEPTH)
        tried += 1
        if d.axis >= 0:
            zero += d.L == 0
            full += d.L == n
    assert tried == 3000 and full == 0
    assert zero > 100


# ---------------------------------------------------------------- non-finite geometry at load

SIX = [[0, 0, 0, 1, 0, 0, 0, 1, 0], [2, 0, 0, 3, 0, 0, 2, 1, 0], [4, 0, 1, 5, 0, 0, 4, 1, 0],
       [6, 0, 0, 7, 0, 2, 6, 1, 0], [8, 1, 0, 9, 0, 0, 8, 1, 3], [10, 0, 0, 11, 0, 0, 10, 1, 0]]


def six_triangles(bad=None):
    lines = []
    for i, t in enumerate(SIX):
        vals = [repr(float(x)) for x in t]
        if i == 3 and bad is not None:
            vals[3] = bad
        lines.append("triangle %s %s\n" % (cases.MATERIALS[i % 5], " ".join(vals)))
    return cases.scene_text(lines)


def test_one_coordinate_of_3e38_loads_like_the_oracle(tmp_path):
    """A single coordinate of 3e38 is finite and so is its triangle's centroid (1e38): nothing in the build
    is undefined.  The root's area overflows to inf, no cost is below it, and the scene is one leaf."""
    p = tmp_path / "huge_coordinate.scene"
    p.write_text(six_triangles("3e38"))
    a, b = O.OracleScene(str(p)).arrays(), R.Scene(str(p)).arrays()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert b["bvh"].shape[0] == 1 and b["bvh"][0, 3] == np.float32(3e38)
    verts = np.array(SIX, np.float32)
    verts[3, 3] = 3e38
    d = ref.decide(*ref.build_input(verts), ref.MAX_DEPTH)
    assert np.isinf(d.own_cost) and d.axis < 0 and d.skipped == [False, False, False]
    p.write_text(six_triangles())                       # the same six without it do split
    assert R.Scene(str(p)).arrays()["bvh"].shape[0] > 1
