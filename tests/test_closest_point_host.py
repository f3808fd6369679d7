"""Closest-point queries on the host (rt_scene_closest_point, rtamd.Scene.closest_point), without a GPU.

* The host twin equals the yardstick (tests/closest_point_ref.py: rt_abi.h's rules op by op in numpy float32) on every
  field of every row, miss rows included, for every scene, point set and bound class.
* The yardstick alone against the brute force over all primitives (the same per-primitive functions): never nearer,
  different on at most 1 % of the finite points, and where different, by rounding error only.
* The inputs do what they are meant to (from the yardstick alone): all seven regions of the triangle rule, stacks past
  the kernel's LDS entries, the big-leaf indirection, ties decided by the index, misses and hits under the bound classes.
* The refit, optional outputs and guard rows, refused arguments, the ABI, the Python wrappers' ValueErrors, and
  signed_distance on a closed cube and a tetrahedron against the exact value.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_ref as CR
import closest_point_scenes as S
import edge_scenes
import refit_ref as RR
import rtamd as R

CLOSEST_POINT_FUNCTIONS = ("rt_query_closest_point", "rt_query_closest_point_host", "rt_scene_closest_point")
EPS32 = float(np.finfo(np.float32).eps)


def _assert_rows(what, got, want, points, fields=S.FIELDS):
    bad = S.differing_rows(got, want, fields)
    assert bad.size == 0, "%s: %d rows differ, first %d (point %r): got %r, want %r" % (
        what, bad.size, bad[0], points[bad[0]], {f: got[f][bad[0]] for f in fields}, {f: want[f][bad[0]] for f in fields})


@pytest.mark.parametrize("scene", S.SCENES)
def test_host_twin_equals_yardstick(scene):
    sc = S.scene(scene)
    for name, (pts, md, res) in S.ref(scene).items():
        for b in S.BOUNDS:
            got = sc.closest_point(pts, None if b == "none" else md)
            assert [got[f].dtype for f in S.FIELDS] == [np.float32, np.int32, np.float32, np.float32]
            _assert_rows("%s/%s max_dist=%s" % (scene, name, b), got, res[b], pts)


def _unit_of(arr, pts, dist):
    """eps32 * (largest absolute coordinate of the scene and the point + distance), per point."""
    lo, hi, _ = S.extent(arr)
    big = max(float(np.abs(lo).max()), float(np.abs(hi).max()))
    return EPS32 * (np.maximum(big, np.abs(pts.astype(np.float64)).max(1)) + dist)


@pytest.mark.parametrize("scene", S.SCENES)
def test_yardstick_against_brute_force(scene):
    """On the yardstick alone, so that the inputs are shown to test something.  The walk's result is the minimum over
    the primitives it tests: dist2 >= the brute force's everywhere; the two differ on at most 1 % of the finite points
    (the prototype and this suite's inputs: 0); where they differ, |distance - brute distance| <= BOUND units of
    eps32 * (largest absolute coordinate + distance), BOUND = twice the largest error the float32 brute force itself
    shows against the float64 brute force on these inputs (a pruning slip mixes one box rounding and one triangle
    rounding of that size; points whose float32 dist2 overflows to +inf, as on `deep`, are left out of the bound and must
    agree exactly).  Measured on these inputs: the float32 brute force is within 1.89 units of the float64 one (big_leaf;
    teapot 0.79), so BOUND is at most 3.8.  The float64 brute force is evaluated only if some point differs."""
    m, arr = S.model(scene), S.scene(scene).arrays()
    total = differ = 0
    for name in S.FINITE_SETS:
        pts, _, res = S.ref(scene)[name]
        got = res["none"]
        b2, bi = m.brute(pts)
        dist_b = np.sqrt(b2)
        assert (got["index"] >= 0).all() and (bi >= 0).all(), (scene, name)
        # distance = sqrtf(best2) is monotone in best2, and best2 >= brute dist2 implies sqrtf(best2) >= sqrtf(brute)
        assert (got["distance"] >= dist_b).all(), (scene, name)
        diff = ~((got["index"] == bi) & CR.same(got["distance"], dist_b))
        total += pts.shape[0]
        differ += int(diff.sum())
        if diff.any():
            fin = np.isfinite(dist_b)                    # a float32 dist2 that overflowed is no rounding error
            assert CR.same(got["distance"][~fin], dist_b[~fin]).all(), (scene, name)
            b64 = np.sqrt(m.brute(pts, np.float64)[0])
            unit = _unit_of(arr, pts, b64)
            bound = 2 * float((np.abs(dist_b.astype(np.float64) - b64) / unit)[fin].max())
            err = (np.abs(got["distance"].astype(np.float64) - dist_b.astype(np.float64)) / unit)[diff & fin]
            print("%s/%s: %d differ, max %.3g units, bound %.3g" % (scene, name, int(diff.sum()), err.max(initial=0), bound))
            assert (err <= bound).all(), (scene, name, float(err.max(initial=0)), bound)
    print("%s: %d of %d finite points differ from the brute force" % (scene, differ, total))
    assert differ <= total // 100


def test_inputs_cover_the_paths():
    """Conditions on the inputs, from the yardstick alone.  A region counts for a point when one of the triangle tests
    of the point's walk falls into it (`tested`): with 300 uniform points in and around a closed box the ACCEPTED
    triangle's region is the face for most of them, so the accepted regions are counted over all of cornell's sets."""
    uni = S.ref("cornell")["uniform"][2]["none"]
    tested = [int(((uni["tested"] >> r) & 1).sum()) for r in range(7)]
    assert min(tested) >= 10, dict(zip(CR.REGIONS, tested))
    acc = np.concatenate([res["none"]["region"] for _, _, res in S.ref("cornell").values()])
    accepted = np.bincount(acc[acc >= 0], minlength=7)
    assert accepted.min() >= 10, dict(zip(CR.REGIONS, accepted))
    deep = max(int(res["none"]["depth"].max()) for _, _, res in S.ref("deep").values())
    assert deep > CR.LDS_ENTRIES and deep == 29
    assert int(S.ref("teapot")["surface"][2]["none"]["depth"].max()) > 16
    assert int(S.ref("big_leaf")["surface"][2]["none"]["max_leaf"].max()) > CR.INLINE_LEAF
    assert int(S.ref("twins")["over_twins"][2]["none"]["ties"].sum()) >= 1
    for scene in S.SCENES:
        for name, (_, _, res) in S.ref(scene).items():
            idx = res["classes"]["index"]
            assert (idx < 0).any() and (idx >= 0).any(), (scene, name)           # the classes give misses and hits
    ns = S.scene("cornell_plus").view.sphere_count
    idx = S.ref("cornell_plus")["uniform"][2]["none"]["index"]
    assert ns > 0 and (idx < ns).any() and (idx >= ns).any()                      # spheres and triangles are nearest


@pytest.mark.parametrize("scene", ["cornell", "cornell_plus", "deep", "big_leaf", "twins"])
def test_host_twin_after_refit(scene):
    """After Scene.refit the answers follow the new vertices: the twin reads the scene's current triangles and boxes."""
    path, use_bvh = S.MS.scene_path(scene)
    sc = R.Scene(path, use_bvh=use_bvh, image=S.MS.IMG)
    sc.refit(RR.deform(sc.vertices(), "jitter"))
    ref = CR.ClosestPointRef(sc)
    moved = 0
    for name in ("uniform", "surface", "vertex"):
        pts, md, res = S.ref(scene)[name]
        pts, md = np.ascontiguousarray(pts[:100]), np.ascontiguousarray(md[:100])
        for b, mdist in (("none", None), ("classes", md)):
            want = ref.batch(pts, mdist)
            _assert_rows("%s/%s refit max_dist=%s" % (scene, name, b), sc.closest_point(pts, mdist), want, pts)
        moved += S.differing_rows(want, {f: res["classes"][f][:100] for f in S.FIELDS}).size
    assert moved > 0


def _buffers(n):
    return {"distance": np.full(n + 1, 7.5, np.float32), "index": np.full(n + 1, 77, np.int32),
            "point": np.full((n + 1, 3), 7.5, np.float32), "uv": np.full((n + 1, 2), 7.5, np.float32)}


GIVEN = (S.FIELDS, ("distance",), ("index",), ("point",), ("uv",), (), ("index", "uv"))


def check_outputs(call, pts, want):
    """call(co) runs the raw function on an RtClosestPointOut: a NULL pointer's array is untouched, nothing is written
    past n rows, the given ones are exact."""
    n = pts.shape[0]
    for given in GIVEN:
        buf = _buffers(n)
        fill = {x: v.copy() for x, v in buf.items()}
        co = R.RtClosestPointOut(**{x: R._ptr(buf[x]) for x in given})
        call(co)
        for x in S.FIELDS:
            assert buf[x][n:].tobytes() == fill[x][n:].tobytes(), (given, x)
            if x in given:
                assert S.differing_rows({x: buf[x][:n]}, want, (x,)).size == 0, (given, x)
            else:
                assert buf[x].tobytes() == fill[x].tobytes(), (given, x)


def test_optional_outputs_and_guard_rows():
    sc = S.scene("cornell_plus")
    pts, md, res = S.ref("cornell_plus")["uniform"]
    f = R.lib().rt_scene_closest_point
    f.argtypes = [R.P, R.P, R.P, R.I32, R.P]

    def call(co):
        assert f(sc.ptr, R._ptr(pts), R._ptr(md), pts.shape[0], C.byref(co)) == 0
    check_outputs(call, pts, res["classes"])


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message():
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_scene_closest_point.argtypes = [P, P, P, I32, P]
    lib.rt_query_closest_point.argtypes = [P, P, P, I32, P, P]
    lib.rt_query_closest_point_host.argtypes = [P, P, P, I32, P]
    sc = S.scene("cornell")
    pts = np.ascontiguousarray(S.sets("cornell")["uniform"][:8])
    d = np.full(8, 7, np.float32)
    co = R.RtClosestPointOut(distance=R._ptr(d))
    p, cp = R._ptr(pts), C.byref(co)
    # a block of zeros stands in for a query object no GPU-less box can create (see test_query_abi.py): the checks
    # come before the object is used and before any HIP call
    obj = R._ptr(np.zeros(1 << 16, np.uint8))
    calls = ((lambda o, *a: lib.rt_scene_closest_point(o, *a), "rt_scene_closest_point", sc.ptr, "null scene"),
             (lambda o, *a: lib.rt_query_closest_point(o, *a, None), "rt_query_closest_point", obj, "null query"),
             (lambda o, *a: lib.rt_query_closest_point_host(o, *a), "rt_query_closest_point_host", obj, "null query"))
    for fn, name, o, null_word in calls:
        _invalid(lib, fn(None, p, None, 8, cp), name + ":", null_word)
        _invalid(lib, fn(o, p, None, -1, cp), name + ":", "negative")
        _invalid(lib, fn(o, None, None, 8, cp), name + ":", "null pointer")
        _invalid(lib, fn(o, p, None, 8, None), name + ":", "null pointer")
        assert fn(o, None, None, 0, None) == 0                                    # n == 0: no pointer touched
    assert (d == 7).all()                                                         # a refused call writes nothing


def test_python_wrappers_convert_nothing_silently():
    import torch
    sc = S.scene("cornell")
    pts = np.ascontiguousarray(S.sets("cornell")["uniform"][:8])
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None       # a library call would raise AttributeError
    for obj in (sc, q):
        for bad in ((pts.astype(np.float64),), (pts[:, :2],), (np.zeros((8, 6), np.float32)[:, ::2],),
                    (pts, np.zeros(7, np.float32)), (pts, np.zeros(8, np.float64)), (pts, None, ("distance", "normal")),
                    (pts, None, "t")):
            with pytest.raises(ValueError):
                obj.closest_point(*bad)
        with pytest.raises(ValueError):
            obj.signed_distance(pts, direction=(1.0, 0.0))
    cases = {"float32": torch.zeros((4, 3), dtype=torch.float64), "shape": torch.zeros((4, 6), dtype=torch.float32),
             "contiguous": torch.zeros((4, 6), dtype=torch.float32)[:, ::2],
             "cuda:0": torch.zeros((4, 3), dtype=torch.float32)}
    for word, x in cases.items():
        with pytest.raises(ValueError, match=word):
            q.closest_point(x)
    assert sc.closest_point(pts, fields=()) == {}
    assert list(sc.closest_point(pts, fields=("uv", "distance"))) == ["distance", "uv"]


def test_header_and_libraries_have_the_closest_point_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(CLOSEST_POINT_FUNCTIONS) <= names and "rt_closest_point_out;" in text
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(CLOSEST_POINT_FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtOpts) == 56
    assert C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8
    assert C.sizeof(R.RtClosestPointOut) == 4 * C.sizeof(C.c_void_p)


# ---------------------------------------------------------------- signed_distance on closed meshes
CUBE = [((-1, -1, -1), (1, -1, -1), (1, 1, -1)), ((-1, -1, -1), (1, 1, -1), (-1, 1, -1)),
        ((-1, -1, 1), (1, 1, 1), (1, -1, 1)), ((-1, -1, 1), (-1, 1, 1), (1, 1, 1)),
        ((-1, -1, -1), (-1, 1, -1), (-1, 1, 1)), ((-1, -1, -1), (-1, 1, 1), (-1, -1, 1)),
        ((1, -1, -1), (1, 1, 1), (1, 1, -1)), ((1, -1, -1), (1, -1, 1), (1, 1, 1)),
        ((-1, -1, -1), (1, -1, 1), (1, -1, -1)), ((-1, -1, -1), (-1, -1, 1), (1, -1, 1)),
        ((-1, 1, -1), (1, 1, -1), (1, 1, 1)), ((-1, 1, -1), (1, 1, 1), (-1, 1, 1))]
_TV = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))
TETRA = [(_TV[0], _TV[1], _TV[2]), (_TV[0], _TV[3], _TV[1]), (_TV[0], _TV[2], _TV[3]), (_TV[1], _TV[3], _TV[2])]
DIRECTION = (0.5773503, 0.5773503, 0.5773503)


def _mesh_scene(tmp_path, name, tris):
    text = edge_scenes.HEADER + "".join(edge_scenes._tri(*t) for t in tris)
    text += "camera position 0 0 6 forward 0 0 -1 up 0 1 0 fov 40\nimage 16 16 1 1 1\n"
    path = os.path.join(str(tmp_path), name + ".scene")
    with open(path, "w") as f:
        f.write(text)
    return R.Scene(path, image=(16, 16, 1, 1))


def _exact(tris, pts):
    """The exact signed distance to a closed convex mesh, float64: the unsigned distance is the minimum over the
    triangles (the triangle rule in float64), the point is inside iff it is behind every face's plane; also the
    smallest distance of the point to a face's plane."""
    V = np.asarray(tris, np.float64)
    rec = np.hstack([V[:, 0], V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]])
    centre = V.reshape(-1, 3).mean(0)
    nrm = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    nrm /= np.sqrt((nrm * nrm).sum(1, keepdims=True))
    nrm *= np.sign(((V[:, 0] - centre) * nrm).sum(1, keepdims=True))           # outward
    sd, off = np.zeros(len(pts)), np.zeros(len(pts))
    for i, p in enumerate(pts.astype(np.float64)):
        d = float(np.sqrt(CR.triangles(p, rec.T, np.float64)[0].min()))
        h = ((p - V[:, 0]) * nrm).sum(1)
        sd[i], off[i] = (-d if (h < 0).all() else d), np.abs(h).min()
    return sd, off


def _grazes(tris, pts, d, margin=0.05):
    """Whether the ray from each point along d passes within `margin` (in barycentric units) of an edge of a triangle
    it reaches, or runs nearly parallel to that triangle's plane (Moeller-Trumbore in float64)."""
    V = np.asarray(tris, np.float64)
    d = np.asarray(d, np.float64)
    out = np.zeros(len(pts), bool)
    for a, b, c in V:
        e1, e2 = b - a, c - a
        h = np.cross(d, e2)
        det = float(h @ e1)
        assert abs(det) > 1e-3                              # the direction is not inside any face's plane
        s = pts.astype(np.float64) - a
        u = (s @ h) / det
        q = np.cross(s, e1)
        v = (q @ d) / det
        t = (q @ e2) / det
        near = lambda x: np.abs(x) < margin
        inside = (u > -margin) & (v > -margin) & (u + v < 1 + margin)
        out |= (t > -margin) & inside & (near(u) | near(v) | near(1 - u - v) | near(t))
    return out


@pytest.mark.parametrize("mesh", ["cube", "tetrahedron"])
def test_signed_distance_on_closed_meshes(mesh, tmp_path):
    """Scene.signed_distance (the composition RayQuery.signed_distance is, on the host twins) against the exact value,
    at seeded points kept 0.05 off every face's plane and whose parity ray stays clear of every edge.  Tolerance: the
    float32 distance is a chain of about 30 roundings of values no larger than (largest coordinate + distance),
    hence 32 eps32 * (largest coordinate + distance)."""
    tris = CUBE if mesh == "cube" else TETRA
    sc = _mesh_scene(tmp_path, mesh, tris)
    assert sc.view.triangle_count == len(tris) and sc.view.sphere_count == 0
    rng = np.random.default_rng(99)
    pts = (rng.random((600, 3)) * 4 - 2).astype(np.float32)
    want, off = _exact(tris, pts)
    keep = (off > 0.05) & ~_grazes(tris, pts, DIRECTION)
    pts, want = np.ascontiguousarray(pts[keep]), want[keep]
    assert pts.shape[0] >= 200 and (want < 0).sum() >= 10 and (want > 0).sum() >= 100
    got = sc.signed_distance(pts)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got < 0, want < 0)
    tol = 32 * EPS32 * (np.abs(pts).max(1) + np.abs(want))
    assert (np.abs(got.astype(np.float64) - want) <= tol).all(), float((np.abs(got - want) / tol).max())
    if mesh == "cube":                                       # the box's closed form
        q = np.abs(pts.astype(np.float64)) - 1
        box = np.sqrt((np.maximum(q, 0) ** 2).sum(1)) + np.minimum(q.max(1), 0)
        assert np.allclose(box, want, rtol=0, atol=1e-12)
