"""Box overlap queries on the GPU: rt_query_overlap_box (rtamd.RayQuery.overlap_box) against its host twin and
against the yardstick (tests/overlap_ref.py).

* every field of every row equals Scene.overlap_box (the host twin) on numpy input and on torch tensors: 2,000 boxes per
  set on the small scenes and 256 on teapot for K in {1, 8, 64}; the first 300 boxes of every set also equal the
  yardstick; with the counters build and without;
* with counters on, the summed Pn, Iv, Tt and sphere tests equal the yardstick's to the unit, for the full walk and for
  the any-only walk (which stops at a box's first member, in the pinned order), and stats() is as specified;
* batch sizes around the wave and workgroup size;
* deep and teapot surface boxes interleaved with invalid and tiny ones in one wave, across the LDS/overflow boundary of
  the stack on deep, at K = 1 and 32; one 2^18-box count-only call;
* overlap_box alternating with nearest_k and occluded on two streams (one scratch, one overflow buffer), and after
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
import overlap_ref as OR
import overlap_scenes as S
import refit_ref as RR
import rtamd as R
from test_overlap_host import check_outputs

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
KS = (1, 8, 64)
N_ANY = 100              # boxes per set whose any-only walk the yardstick steps through


def _need_gpu():
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _twin(scene, name, k):
    """The host twin's answers: (boxes, dict of fields)."""
    b = S.sets(scene)[name]
    return b, S.scene(scene).overlap_box(b, k, fields=OR.FIELDS)


@functools.lru_cache(maxsize=None)
def _any_walks(scene, name):
    """The yardstick's any-only walk of the first N_ANY boxes of a set: (boxes, any (n,) uint8, counters (n, 4))."""
    b = np.ascontiguousarray(S.ref(scene)[name]["boxes"][:N_ANY])
    walks = [S.model(scene).any_walk(x) for x in b]
    return b, np.array([w[0] for w in walks], np.uint8), np.array([w[1] for w in walks], np.int64).reshape(-1, 4)


def _np(got):
    return {k: np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v for k, v in got.items()}


def _assert_same(what, got, want, fields=OR.FIELDS):
    got = _np(got)
    assert tuple(got) == tuple(fields), (what, tuple(got))
    bad = S.differing_rows(got, want, fields) if fields else np.zeros(0, np.int64)
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
    zeros = np.zeros((1, 4), np.int64)
    try:
        for name in S.sets(scene):
            b, want = _twin(scene, name, k)
            what = "%s/%s k=%d" % (scene, name, k)
            _assert_same(what + " numpy", q.overlap_box(b, k, fields=OR.FIELDS), want)
            _assert_stats(what, q, want["count"])
            got = q.overlap_box(_cuda(b), k, fields=OR.FIELDS)
            assert all(g.is_cuda and g.is_contiguous() for g in got.values())
            assert [g.dtype for g in got.values()] == [torch.int32, torch.int32, torch.uint8]
            _assert_same(what + " torch", got, want)
        for name, r in S.ref(scene).items():
            res = S.rows(scene, name, k)
            what = "%s/%s k=%d yardstick" % (scene, name, k)
            _assert_same(what, q.overlap_box(r["boxes"], k, fields=OR.FIELDS), res)
            _assert_stats(what, q, res["count"], res["ctr"] if counters else zeros)
            if k != 1:
                continue
            b, any_want, ctr = _any_walks(scene, name)          # the any-only walk: the pinned order's counters
            what = "%s/%s any-only" % (scene, name)
            _assert_same(what, q.overlap_box(_cuda(b), k, fields=("any",)), {"any": any_want}, ("any",))
            _assert_stats(what, q, any_want, ctr if counters else zeros)
            _assert_same(what + " numpy", q.overlap_box(b, k, fields=("any",)), {"any": any_want}, ("any",))
            _assert_stats(what + " numpy", q, any_want, ctr if counters else zeros)
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres", "twins"])
def test_batch_sizes(scene):
    _need_gpu()
    q = R.RayQuery(S.scene(scene))
    try:
        b_all, want = _twin(scene, "surface", 8)
        for n in (0, 1, 63, 64, 65, 2037):
            rep = np.arange(n) % b_all.shape[0]
            b = np.ascontiguousarray(b_all[rep])
            got = q.overlap_box(b, 8, fields=OR.FIELDS)
            assert got["index"].shape == (n, 8) and got["count"].shape == (n,) and got["any"].shape == (n,)
            _assert_same("%s n=%d" % (scene, n), got, {f: want[f][rep] for f in OR.FIELDS})
            got = q.overlap_box(_cuda(b), 8, fields=OR.FIELDS)
            _assert_same("%s n=%d torch" % (scene, n), got, {f: want[f][rep] for f in OR.FIELDS})
    finally:
        q.close()


def _weave(parts):
    """Row i of each array in turn."""
    a = np.stack(parts, 1)
    return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))


@functools.lru_cache(maxsize=None)
def _woven(scene, k):
    """256 surface boxes of the scene (deep stacks), invalid boxes and tiny ones (1e-6 D around surface points),
    interleaved: every wave holds all three.  -> (boxes, twin's rows)."""
    n = 256
    surface = S.sets(scene)["surface"][:n]
    c = (surface[:, 0:3].astype(np.float64) + surface[:, 3:6]) / 2
    tiny = S._box(c, np.full((n, 3), 1e-6 * S.diagonal(scene)))
    b = _weave([surface, S.sets(scene)["invalid"][:n], tiny])
    return b, S.scene(scene).overlap_box(b, k, fields=OR.FIELDS)


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", ["deep", "teapot"])
def test_deep_stack(scene, counters):
    """deep's surface boxes hold more than the 16 LDS entries; teapot's reach the 15 its tree allows under the pinned
    order (test_overlap_host.test_inputs_cover_the_paths)."""
    _need_gpu()
    depth = int(S.rows(scene, "surface", 1)["depth"][:256].max())
    assert depth > OR.ANY_LDS_ENTRIES if scene == "deep" else depth == 15
    q = R.RayQuery(S.scene(scene), counters=counters)
    try:
        for k in (1, 32):
            b, want = _woven(scene, k)
            what = "%s deep stack k=%d" % (scene, k)
            _assert_same(what, q.overlap_box(b, k, fields=OR.FIELDS), want)
            _assert_stats(what, q, want["count"])
            _assert_same(what + " torch", q.overlap_box(_cuda(b), k, fields=OR.FIELDS), want)
            _assert_same(what + " any", q.overlap_box(_cuda(b), k, fields=("any",)), want, ("any",))
            _assert_stats(what + " any", q, want["count"])
    finally:
        q.close()


def test_large_count_only_call():
    """2^18 boxes = 1024 workgroups of 256 lanes, count only: a fixed permutation of deep's uniform, surface and invalid
    boxes, interleaved and tiled."""
    _need_gpu()
    parts = [_twin("deep", name, 1) for name in ("uniform", "surface", "invalid")]
    b, cnt = _weave([p[0] for p in parts]), _weave([p[1]["count"] for p in parts])
    idx = np.random.default_rng(5).permutation(b.shape[0])[np.arange(1 << 18) % b.shape[0]]
    q = R.RayQuery(S.scene("deep"))
    try:
        got = q.overlap_box(_cuda(np.ascontiguousarray(b[idx])), 1, fields=("count",))
        _assert_same("deep/2^18 count only", got, {"count": cnt[idx]}, ("count",))
        _assert_stats("deep/2^18 count only", q, cnt[idx])
    finally:
        q.close()


def test_alternating_streams_and_update():
    """overlap_box, nearest_k and occluded alternate on two torch streams on one object: they share the slots, the queue
    words and the one overflow buffer (the other queries' own answers come from a second object, one call at a time).
    Then overlap_box after RayQuery.update, against the refitted host scene."""
    _need_gpu()
    torch.cuda.set_device(0)
    b, want = _woven("deep", 8)
    rays = edge_scenes.interleaved(edge_scenes.axis_plus(1024), edge_scenes.solid_minus(1024), edge_scenes.tilted_plus(1024))
    tm = np.full(rays.shape[0], 1e4, np.float32)
    pts = np.ascontiguousarray(S.CS.sets("deep")["surface"][:1024])
    b_t, rays_t, tm_t, pts_t = _cuda(b), _cuda(rays), _cuda(tm), _cuda(pts)
    q0 = R.RayQuery(S.scene("deep"))
    try:
        nk = q0.nearest_k(pts, 8)
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
                outs.append(("overlap", q.overlap_box(b_t, 8, fields=OR.FIELDS)))
            with torch.cuda.stream(s2):
                outs.append(("nearest", q.nearest_k(pts_t, 8)))
            with torch.cuda.stream(s1):
                outs.append(("occluded", q.occluded(rays_t, tm_t)))
            with torch.cuda.stream(s2):
                outs.append(("overlap", q.overlap_box(b_t, 8, fields=OR.FIELDS)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "overlap":
                _assert_same("streams overlap_box", r, want)
            elif kind == "nearest":
                assert S.CS.differing_rows(_np(r), nk, tuple(nk)).size == 0
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
            bx, old = _twin(scene, "surface", 8)
            before = q.overlap_box(bx, 8, fields=OR.FIELDS)
            _assert_same("%s before update" % scene, before, old)
            q.update(_cuda(V))
            new = moved.overlap_box(bx, 8, fields=OR.FIELDS)
            assert S.differing_rows(before, new).size > 0
            _assert_same("%s after update" % scene, q.overlap_box(bx, 8, fields=OR.FIELDS), new)
            _assert_same("%s after update, torch" % scene, q.overlap_box(_cuda(bx), 8, fields=OR.FIELDS), new)
        finally:
            q.close()


@pytest.mark.parametrize("k", [1, 8])
def test_optional_outputs(k):
    """The raw _host call on pattern-filled buffers with guard rows: an output whose pointer is NULL is not written, the
    others are exact, and with no output the call only traverses and counts; the same choices through the device-pointer
    call.  The counters are the full walk's except with `any` alone, where they are the any-only walk's."""
    _need_gpu()
    torch.cuda.set_device(0)
    b, want = S.ref("cornell_plus")["uniform"]["boxes"], S.rows("cornell_plus", "uniform", k)
    m = S.model("cornell_plus")
    any_ctr = np.array([m.any_walk(x)[1] for x in b], np.int64)
    q = R.RayQuery(S.scene("cornell_plus"), counters=True)
    f = q.L.rt_query_overlap_box_host
    f.argtypes = [R.P, R.P, R.I32, R.I32, R.P]
    try:
        def call(oo):
            assert f(q.h, R._ptr(b), b.shape[0], k, C.byref(oo)) == 0, q.L.rt_last_error()
            any_only = bool(oo.any) and not oo.index and not oo.count
            _assert_stats("outputs", q, want["count"], any_ctr if any_only else want["ctr"])
        check_outputs(call, b.shape[0], k, want)
        for given in (("index",), ("count",), ("any",), (), ("index", "any"), OR.FIELDS):
            got = q.overlap_box(_cuda(b), k, fields=given)
            _assert_same("device outputs %s" % (given,), got, want, given)
            _assert_stats("device outputs %s" % (given,), q, want["count"], any_ctr if given == ("any",) else want["ctr"])
    finally:
        q.close()
