"""Range queries on the GPU: rt_query_nearest_k (rtamd.RayQuery.nearest_k) against its host twin and against
the yardstick (tests/nearest_k_ref.py).

* every field of every row equals Scene.nearest_k (the host twin) bit for bit on numpy input and on torch tensors
  (max_dist then a tensor too): 2,000 points per set under the bounded radius classes for K in {1, 8, 64}, the unbounded
  classes and max_dist = None on the small scenes and on 64 teapot points; the first 300 points of every set also equal
  the yardstick; with the counters build and without;
* with counters on, the summed Pn, Iv, Tt and sphere tests equal the yardstick's to the unit (the full walk does not
  depend on the order), and stats() is as specified;
* batch sizes around the wave and workgroup size;
* deep and teapot surface points, whose stacks pass the 16 LDS entries into the overflow buffer, interleaved with
  shallow ones in one wave, at K = 1 and 32; a 2^20-point call, a grid as large as the library launches, at K = 2;
* nearest_k alternating with closest_point and occluded on two streams (one scratch, one overflow buffer), and after
  update;
* optional outputs: each alone and none.
The yardstick's and the twin's answers are computed once per process and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import edge_scenes
import nearest_k_ref as NR
import nearest_k_scenes as S
import refit_ref as RR
import rtamd as R
from test_nearest_k_host import check_outputs

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
KS = (1, 8, 64)


def _need_gpu():
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _twin(scene, name, k):
    """The host twin's bounded answers: (points (N_SET, 3), max_dist, dict of fields)."""
    pts, md = S.sets(scene)[name], S.radii(scene)[name]
    return pts, md, S.scene(scene).nearest_k(pts, k, md)


@functools.lru_cache(maxsize=None)
def _twin_unbounded(scene, name, k):
    """The host twin's answers under the unbounded classes (max_dist = None gives the same rows: test_nearest_k_host)."""
    pts, md = S.unbounded(scene)[name]
    return pts, md, S.scene(scene).nearest_k(pts, k, md)


def _unbounded_sets(scene):
    return S.TEAPOT_GPU_SETS if scene == "teapot" else tuple(S.sets(scene))


def _np(got):
    return {k: np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v for k, v in got.items()}


def _assert_same(what, got, want, fields=NR.FIELDS):
    got = _np(got)
    assert tuple(got) == tuple(fields), (what, tuple(got))
    bad = S.differing_rows(got, want, fields)
    assert bad.size == 0, "%s: %d rows differ, first %d: gpu %r, want %r" % (
        what, bad.size, bad[0], {f: got[f][bad[0]] for f in fields}, {f: want[f][bad[0]] for f in fields})


def _assert_stats(what, q, count, ctr=None):
    st = q.stats()
    n, hits = count.shape[0], int((count >= 1).sum())
    assert st["live_segments"] == n and st["hits"] == hits and st["misses"] == n - hits, (what, st)
    assert st["hits_sphere"] == 0, (what, st)
    if ctr is not None:
        want = [int(v) for v in ctr.sum(0)]
        assert [st[x] for x in COUNTERS] == want, "%s: Pn/Iv/Tt/sphere tests: gpu %s yardstick %s" % (
            what, [st[x] for x in COUNTERS], want)


def _cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("scene", S.SCENES)
def test_equals_host_twin_and_yardstick(scene, k, counters):
    _need_gpu()
    torch.cuda.set_device(0)
    q = R.RayQuery(S.scene(scene), counters=counters)
    try:
        for name in S.sets(scene):
            pts, md, want = _twin(scene, name, k)
            what = "%s/%s k=%d bounded" % (scene, name, k)
            _assert_same(what + " numpy", q.nearest_k(pts, k, md), want)
            _assert_stats(what, q, want["count"])
            got = q.nearest_k(_cuda(pts), k, _cuda(md))
            assert all(g.is_cuda and g.is_contiguous() for g in got.values())
            assert [g.dtype for g in got.values()] == [torch.float32, torch.int32, torch.float32, torch.int32]
            _assert_same(what + " torch", got, want)
        for name in _unbounded_sets(scene):
            pts, md, want = _twin_unbounded(scene, name, k)
            what = "%s/%s k=%d unbounded" % (scene, name, k)
            _assert_same(what + " classes torch", q.nearest_k(_cuda(pts), k, _cuda(md)), want)
            _assert_same(what + " none numpy", q.nearest_k(pts, k), want)
            if scene != "teapot":                       # a teapot call tests every triangle for every point
                _assert_same(what + " classes numpy", q.nearest_k(pts, k, md), want)
                _assert_same(what + " none torch", q.nearest_k(_cuda(pts), k), want)
            _assert_stats(what, q, want["count"])
        for name, r in S.ref(scene).items():
            for run in ("bounded", "classes"):
                if run == "classes" and name not in _unbounded_sets(scene):
                    continue
                pts, md = (r["points"], r["max_dist"]) if run == "bounded" else (r["u_points"], r["u_max_dist"])
                res = S.rows(scene, name, run, k)
                what = "%s/%s k=%d %s yardstick" % (scene, name, k, run)
                _assert_same(what, q.nearest_k(pts, k, md), res)
                _assert_stats(what, q, res["count"], res["ctr"] if counters else np.zeros((1, 4), np.int64))
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres", "twins"])
def test_batch_sizes(scene):
    _need_gpu()
    name = "over_twins" if scene == "twins" else "surface"
    q = R.RayQuery(S.scene(scene))
    try:
        pts_all, md_all, want = _twin(scene, name, 8)
        for n in (0, 1, 63, 64, 65, 2037):
            rep = np.arange(n) % pts_all.shape[0]
            pts, md = np.ascontiguousarray(pts_all[rep]), np.ascontiguousarray(md_all[rep])
            got = q.nearest_k(pts, 8, md)
            assert got["distance"].shape == (n, 8) and got["point"].shape == (n, 8, 3) and got["count"].shape == (n,)
            _assert_same("%s n=%d" % (scene, n), got, {f: want[f][rep] for f in NR.FIELDS})
            got = q.nearest_k(_cuda(pts), 8, _cuda(md))
            _assert_same("%s n=%d torch" % (scene, n), got, {f: want[f][rep] for f in NR.FIELDS})
    finally:
        q.close()


def _weave(parts):
    """Row i of each array in turn."""
    a = np.stack(parts, 1)
    return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))


@functools.lru_cache(maxsize=None)
def _deep_points(scene, k):
    """Points of a deep-stack and a shallow set of the scene, interleaved: every wave holds both.  deep: its uniform
    points under the unbounded classes (every triangle of the 29-deep chain) and its surface points; teapot: 1,024
    surface points (stacks past 16 under 2e-4 D) and uniform points, bounded.  -> (points, max_dist, twin's rows)."""
    if scene == "deep":
        parts = [_twin_unbounded(scene, "uniform", k), _twin_unbounded(scene, "surface", k)]
        n = S.N_UNBOUNDED
    else:
        parts = [_twin(scene, "surface", k), _twin(scene, "uniform", k)]
        n = 1024
    return (_weave([p[0][:n] for p in parts]), _weave([p[1][:n] for p in parts]),
            {f: _weave([p[2][f][:n] for p in parts]) for f in NR.FIELDS})


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", ["deep", "teapot"])
def test_deep_stack(scene, counters):
    _need_gpu()
    run = ("uniform", "classes") if scene == "deep" else ("surface", "bounded")
    depth = S.rows(scene, run[0], run[1], 1)["depth"]
    assert int(depth.max()) > NR.ANY_LDS_ENTRIES                                  # past the LDS entries
    q = R.RayQuery(S.scene(scene), counters=counters)
    try:
        for k in (1, 32):
            pts, md, want = _deep_points(scene, k)
            what = "%s deep stack k=%d" % (scene, k)
            _assert_same(what, q.nearest_k(pts, k, md), want)
            _assert_stats(what, q, want["count"])
            _assert_same(what + " torch", q.nearest_k(_cuda(pts), k, _cuda(md)), want)
    finally:
        q.close()


def test_whole_grid():
    """2^20 points = 4096 workgroups of 256 lanes, more than the library launches (CUs x resident workgroups per CU), so
    the grid is `blocks` and its last lanes address the end of the overflow buffer.  The points are a fixed permutation
    of deep's uniform and surface points under the bounded classes (small radii), interleaved and tiled; K = 2."""
    _need_gpu()
    parts = [_twin("deep", "uniform", 2), _twin("deep", "surface", 2)]
    pts, md = _weave([p[0] for p in parts]), _weave([p[1] for p in parts])
    want = {f: _weave([p[2][f] for p in parts]) for f in NR.FIELDS}
    idx = np.random.default_rng(5).permutation(pts.shape[0])[np.arange(1 << 20) % pts.shape[0]]
    for counters in (True, False):
        q = R.RayQuery(S.scene("deep"), counters=counters)
        try:
            got = q.nearest_k(np.ascontiguousarray(pts[idx]), 2, np.ascontiguousarray(md[idx]))
            _assert_same("deep/whole grid", got, {f: want[f][idx] for f in NR.FIELDS})
            _assert_stats("deep/whole grid", q, want["count"][idx])
        finally:
            q.close()


def test_alternating_streams_and_update():
    """nearest_k, closest_point and occluded alternate on two torch streams on one object: they share the slots, the
    queue words and the one overflow buffer (the other queries' own answers come from a second object, one call at a
    time).  Then nearest_k after RayQuery.update, against the refitted host scene."""
    _need_gpu()
    torch.cuda.set_device(0)
    pts, md, want = _deep_points("deep", 8)
    rays = edge_scenes.interleaved(edge_scenes.axis_plus(1024), edge_scenes.solid_minus(1024), edge_scenes.tilted_plus(1024))
    tm = np.full(rays.shape[0], 1e4, np.float32)
    cp_pts, cp_md = S.sets("deep")["surface"], S.radii("deep")["surface"]
    pts_t, md_t, cp_pts_t, cp_md_t = _cuda(pts), _cuda(md), _cuda(cp_pts), _cuda(cp_md)
    rays_t, tm_t = _cuda(rays), _cuda(tm)
    q0 = R.RayQuery(S.scene("deep"))
    try:
        cp = q0.closest_point(cp_pts, cp_md)
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
                outs.append(("nearest", q.nearest_k(pts_t, 8, md_t)))
            with torch.cuda.stream(s2):
                outs.append(("point", q.closest_point(cp_pts_t, cp_md_t)))
            with torch.cuda.stream(s1):
                outs.append(("occluded", q.occluded(rays_t, tm_t)))
            with torch.cuda.stream(s2):
                outs.append(("nearest", q.nearest_k(pts_t, 8, md_t)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "nearest":
                _assert_same("streams nearest_k", r, want)
            elif kind == "point":
                assert S.CS.differing_rows(_np(r), cp).size == 0
            else:
                assert np.array_equal(r.cpu().numpy(), occ)
    finally:
        q.close()
    for scene in ("teapot", "twins"):
        path, use_bvh = S.CS.MS.scene_path(scene)
        moved = R.Scene(path, use_bvh=use_bvh, image=S.CS.MS.IMG)
        V = RR.deform(moved.vertices(), "jitter")
        q = R.RayQuery(moved)                       # resident: the undeformed geometry
        moved.refit(V)                              # the host scene moves; q keeps its own copy until update
        try:
            p, mdist, old = _twin(scene, "surface", 8)
            before = q.nearest_k(p, 8, mdist)
            _assert_same("%s before update" % scene, before, old)
            q.update(_cuda(V))
            new = moved.nearest_k(p, 8, mdist)
            assert S.differing_rows(before, new).size > 0
            _assert_same("%s after update" % scene, q.nearest_k(p, 8, mdist), new)
            _assert_same("%s after update, torch" % scene, q.nearest_k(_cuda(p), 8, _cuda(mdist)), new)
        finally:
            q.close()


@pytest.mark.parametrize("k", [1, 8])
def test_optional_outputs(k):
    """The raw _host call on pattern-filled buffers: an output whose pointer is NULL is not written, the others are
    exact, and with no output the call only traverses and counts; the same choices through the device-pointer call
    (distance, index or point alone keeps the missing list halves in the object's scratch)."""
    _need_gpu()
    torch.cuda.set_device(0)
    r = S.ref("cornell_plus")["uniform"]
    pts, md, want = r["points"], r["max_dist"], S.rows("cornell_plus", "uniform", "bounded", k)
    q = R.RayQuery(S.scene("cornell_plus"), counters=True)
    f = q.L.rt_query_nearest_k_host
    f.argtypes = [R.P, R.P, R.P, R.I32, R.I32, R.P]
    try:
        def call(no):
            assert f(q.h, R._ptr(pts), R._ptr(md), pts.shape[0], k, C.byref(no)) == 0, q.L.rt_last_error()
            _assert_stats("outputs", q, want["count"], want["ctr"])
        check_outputs(call, pts.shape[0], k, want)
        for given in (("count",), ("distance",), ("index",), ("point",), (), ("index", "point"), NR.FIELDS):
            got = q.nearest_k(_cuda(pts), k, _cuda(md), fields=given)
            _assert_same("device outputs %s" % (given,), got, want, given)
            _assert_stats("device outputs %s" % (given,), q, want["count"], want["ctr"])
    finally:
        q.close()
