"""Closest-point queries on the GPU: rt_query_closest_point (rtamd.RayQuery.closest_point) against its host
twin and against the yardstick (tests/closest_point_ref.py).

* every field of every row equals Scene.closest_point (the host twin) bit for bit on numpy input and on torch tensors
  (max_dist then a tensor too), 2,000 points per set (20,000 for teapot's uniform set), without max_dist and with the
  bound classes, with the counters build and without; the first 300 points also equal the yardstick;
* with counters on, the summed Pn, Iv, Tt and sphere tests equal the yardstick's to the unit (the order is pinned), and
  stats() is as specified;
* batch sizes around the wave and workgroup size;
* deep and teapot surface points, whose stacks pass the 8 LDS entries into the overflow buffer, interleaved with shallow
  ones in one wave; a 2^20-point call, a grid as large as the library launches;
* closest_point alternating with closest and occluded on two streams (one scratch, one overflow buffer), and after
  update;
* optional outputs: each alone and none.
The yardstick's and the twin's answers are computed once per process and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import closest_point_ref as CR
import closest_point_scenes as S
import edge_scenes
import refit_ref as RR
import rtamd as R
from test_closest_point_host import check_outputs

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")


def _need_gpu():
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _twin(scene):
    """The host twin's answers, once per scene: {(set, bound): (points, max_dist or None, dict of fields)}."""
    sc = S.scene(scene)
    out = {}
    for name, pts in S.sets(scene).items():
        none = sc.closest_point(pts)
        md = S.bound_classes(none["distance"])
        out[(name, "none")] = (pts, None, none)
        out[(name, "classes")] = (pts, md, sc.closest_point(pts, md))
    return out


def _np(got):
    return {k: np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v for k, v in got.items()}


def _assert_same(what, got, want, fields=S.FIELDS):
    got = _np(got)
    assert tuple(got) == tuple(fields), (what, tuple(got))
    bad = S.differing_rows(got, want, fields)
    assert bad.size == 0, "%s: %d rows differ, first %d: gpu %r, want %r" % (
        what, bad.size, bad[0], {f: got[f][bad[0]] for f in fields}, {f: want[f][bad[0]] for f in fields})


def _assert_stats(what, q, scene, index, ctr=None):
    st = q.stats()
    n, ns = index.shape[0], S.scene(scene).view.sphere_count
    hits = int((index >= 0).sum())
    assert st["live_segments"] == n and st["hits"] == hits and st["misses"] == n - hits, (what, st)
    assert st["hits_sphere"] == int(((index >= 0) & (index < ns)).sum()), (what, st)
    if ctr is not None:
        want = [int(v) for v in ctr.sum(0)]
        assert [st[x] for x in COUNTERS] == want, "%s: Pn/Iv/Tt/sphere tests: gpu %s yardstick %s" % (
            what, [st[x] for x in COUNTERS], want)


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", S.SCENES)
def test_equals_host_twin_and_yardstick(scene, counters):
    _need_gpu()
    torch.cuda.set_device(0)
    q = R.RayQuery(S.scene(scene), counters=counters)
    try:
        for (name, b), (pts, md, want) in _twin(scene).items():
            what = "%s/%s max_dist=%s" % (scene, name, b)
            _assert_same(what + " numpy", q.closest_point(pts, md), want)
            _assert_stats(what, q, scene, want["index"])
            pts_t = torch.from_numpy(pts).cuda()
            got = q.closest_point(pts_t, None if md is None else torch.from_numpy(md).cuda())
            assert all(g.device == pts_t.device and g.is_contiguous() for g in got.values())
            assert [g.dtype for g in got.values()] == [torch.float32, torch.int32, torch.float32, torch.float32]
            _assert_same(what + " torch", got, want)
        for name, (pts, md, res) in S.ref(scene).items():
            for b in S.BOUNDS:
                what = "%s/%s max_dist=%s yardstick" % (scene, name, b)
                _assert_same(what, q.closest_point(pts, None if b == "none" else md), res[b])
                ctr = res[b]["ctr"] if counters else np.zeros((1, 4), np.int64)
                _assert_stats(what, q, scene, res[b]["index"], ctr)
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres", "twins"])
def test_batch_sizes(scene):
    _need_gpu()
    name = "over_twins" if scene == "twins" else "surface"
    q = R.RayQuery(S.scene(scene))
    try:
        for b in S.BOUNDS:
            pts_all, md_all, want = _twin(scene)[(name, b)]
            for n in (0, 1, 63, 64, 65, 2037):
                rep = np.arange(n) % pts_all.shape[0]
                pts = np.ascontiguousarray(pts_all[rep])
                md = None if md_all is None else np.ascontiguousarray(md_all[rep])
                got = q.closest_point(pts, md)
                assert got["distance"].shape == (n,) and got["point"].shape == (n, 3) and got["uv"].shape == (n, 2)
                _assert_same("%s n=%d max_dist=%s" % (scene, n, b), got, {f: want[f][rep] for f in S.FIELDS})
    finally:
        q.close()


def _weave(parts):
    """Row i of each array in turn."""
    a = np.stack(parts, 1)
    return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))


@functools.lru_cache(maxsize=None)
def _deep_points(scene):
    """1,024 points of each of a deep-stack and a shallow set of the scene, interleaved: every wave holds both."""
    deep, shallow = ("uniform", "surface") if scene == "deep" else ("surface", "uniform")
    tw = _twin(scene)
    out = {}
    for b in S.BOUNDS:
        parts = [tw[(k, b)] for k in (deep, shallow)]
        pts = _weave([p[0][:1024] for p in parts])
        md = None if b == "none" else _weave([p[1][:1024] for p in parts])
        out[b] = (pts, md, {f: _weave([p[2][f][:1024] for p in parts]) for f in S.FIELDS})
    return deep, out


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", ["deep", "teapot"])
def test_deep_stack(scene, counters):
    _need_gpu()
    deep, cases = _deep_points(scene)
    depth = S.ref(scene)[deep][2]["none"]["depth"]
    assert int(depth.max()) > (2 if scene == "deep" else 1) * CR.LDS_ENTRIES      # past the LDS entries
    q = R.RayQuery(S.scene(scene), counters=counters)
    try:
        for b, (pts, md, want) in cases.items():
            what = "%s deep stack max_dist=%s" % (scene, b)
            _assert_same(what, q.closest_point(pts, md), want)
            _assert_stats(what, q, scene, want["index"])
    finally:
        q.close()


def test_whole_grid():
    """2^20 points = 4096 workgroups of 256 lanes, more than the library launches (CUs x resident workgroups per CU), so
    the grid is `blocks` and its last lanes address the end of the overflow buffer.  The points are a fixed permutation
    of the 2,048 interleaved deep points, tiled."""
    _need_gpu()
    _, cases = _deep_points("deep")
    for counters, b in ((True, "none"), (False, "classes")):
        pts, md, want = cases[b]
        idx = np.random.default_rng(5).permutation(pts.shape[0])[np.arange(1 << 20) % pts.shape[0]]
        q = R.RayQuery(S.scene("deep"), counters=counters)
        try:
            got = q.closest_point(np.ascontiguousarray(pts[idx]), None if md is None else np.ascontiguousarray(md[idx]))
            what = "deep/whole grid max_dist=%s" % b
            _assert_same(what, got, {f: want[f][idx] for f in S.FIELDS})
            _assert_stats(what, q, "deep", want["index"][idx])
        finally:
            q.close()


def test_alternating_streams_and_update():
    """closest_point, closest and occluded alternate on two torch streams on one object: they share the slots and lay
    out the one overflow buffer differently (the ray queries' own answers come from a second object, one call at a
    time).  Then closest_point after RayQuery.update, against the refitted host scene."""
    _need_gpu()
    torch.cuda.set_device(0)
    _, cases = _deep_points("deep")
    pts, md, want = cases["classes"]
    rays = edge_scenes.interleaved(edge_scenes.axis_plus(1024), edge_scenes.solid_minus(1024), edge_scenes.tilted_plus(1024))
    tm = np.full(rays.shape[0], 1e4, np.float32)
    pts_t, md_t = torch.from_numpy(pts).cuda(), torch.from_numpy(md).cuda()
    rays_t, tm_t = torch.from_numpy(rays).cuda(), torch.from_numpy(tm).cuda()
    q0 = R.RayQuery(S.scene("deep"))
    try:
        t_c, i_c = q0.closest(rays)
        occ = q0.occluded(rays, tm)
    finally:
        q0.close()
    torch.cuda.synchronize()
    q = R.RayQuery(S.scene("deep"))
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for _ in range(3):
            with torch.cuda.stream(s1):
                outs.append(("point", q.closest_point(pts_t, md_t)))
            with torch.cuda.stream(s2):
                outs.append(("closest", q.closest(rays_t)))
            with torch.cuda.stream(s1):
                outs.append(("occluded", q.occluded(rays_t, tm_t)))
            with torch.cuda.stream(s2):
                outs.append(("point", q.closest_point(pts_t, md_t)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "point":
                _assert_same("streams closest_point", r, want)
            elif kind == "closest":
                assert CR.same(r[0].cpu().numpy(), t_c).all() and np.array_equal(r[1].cpu().numpy(), i_c)
            else:
                assert np.array_equal(r.cpu().numpy(), occ)
    finally:
        q.close()
    for scene in ("teapot", "twins"):
        path, use_bvh = S.MS.scene_path(scene)
        moved = R.Scene(path, use_bvh=use_bvh, image=S.MS.IMG)
        V = RR.deform(moved.vertices(), "jitter")
        q = R.RayQuery(moved)                       # resident: the undeformed geometry
        moved.refit(V)                              # the host scene moves; q keeps its own copy until update
        try:
            p, mdist, old = _twin(scene)[("surface", "classes")]
            before = q.closest_point(p, mdist)
            _assert_same("%s before update" % scene, before, old)
            q.update(torch.from_numpy(V).cuda())
            new = moved.closest_point(p, mdist)
            assert S.differing_rows(before, new).size > 0
            _assert_same("%s after update" % scene, q.closest_point(p, mdist), new)
            _assert_same("%s after update, torch" % scene,
                         q.closest_point(torch.from_numpy(p).cuda(), torch.from_numpy(mdist).cuda()), new)
        finally:
            q.close()


def test_optional_outputs():
    """The raw _host call on pattern-filled buffers: an output whose pointer is NULL is not written, the others are
    exact, and with no output the call only traverses and counts; the same choices through the device-pointer call."""
    _need_gpu()
    torch.cuda.set_device(0)
    pts, md, res = S.ref("cornell_plus")["uniform"]
    want = res["classes"]
    q = R.RayQuery(S.scene("cornell_plus"), counters=True)
    f = q.L.rt_query_closest_point_host
    f.argtypes = [R.P, R.P, R.P, R.I32, R.P]
    try:
        def call(co):
            assert f(q.h, R._ptr(pts), R._ptr(md), pts.shape[0], C.byref(co)) == 0, q.L.rt_last_error()
            _assert_stats("outputs", q, "cornell_plus", want["index"], want["ctr"])
        check_outputs(call, pts, want)
        pts_t, md_t = torch.from_numpy(pts).cuda(), torch.from_numpy(md).cuda()
        for given in (("distance",), ("index",), ("point",), ("uv",), (), ("index", "uv")):
            got = q.closest_point(pts_t, md_t, fields=given)
            _assert_same("device outputs %s" % (given,), got, want, given)
            _assert_stats("device outputs %s" % (given,), q, "cornell_plus", want["index"], want["ctr"])
    finally:
        q.close()


def test_signed_distance_matches_the_host_composition():
    """RayQuery.signed_distance on the GPU equals Scene.signed_distance (both queries are bit-exact twins), numpy and
    torch."""
    _need_gpu()
    torch.cuda.set_device(0)
    pts = np.ascontiguousarray(S.sets("teapot")["uniform"][:2000])
    want = S.scene("teapot").signed_distance(pts)
    assert (want < 0).any() and (want > 0).any()
    q = R.RayQuery(S.scene("teapot"))
    try:
        assert CR.same(q.signed_distance(pts), want).all()
        got = q.signed_distance(torch.from_numpy(pts).cuda())
        assert got.dtype == torch.float32 and CR.same(got.cpu().numpy(), want).all()
    finally:
        q.close()
