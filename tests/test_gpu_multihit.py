"""Multi-hit queries on the GPU: rt_query_multi_hit (rtamd.RayQuery.multi_hit) against its host twin and
against the yardstick (tests/multihit_ref.py).

* every field -- count and all K entries of every row, padding included -- equals Scene.multi_hit (the host twin) bit
  for bit on numpy input and on torch tensors, 2,000 rays per set (20,000 for teapot's random set), tmax = None and the
  bound classes, K in {1, 2, 8, 64}, with the counters build and without; the first 300 rays also equal MultiHitRef;
* with counters on, the summed Pn, Iv, Tt and sphere tests equal the yardstick's to the unit (no exit: the full
  traversal's, on every ray), and stats() is as specified;
* batch sizes around the wave and workgroup size;
* the deep chain: rays whose stacks pass the 16 LDS entries into the overflow buffer with no early exit, at K = 1 and
  K = 32 (truncated rows: solid_plus crosses 60 triangles), and a grid as large as the library launches;
* multi_hit alternating with closest and occluded on two streams (one overflow buffer, one scratch), and after update;
* optional outputs: count only, t only, index only, none.
The yardstick's and the twin's answers are computed once per process and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import multihit_ref as M
import multihit_scenes as S
import refit_ref as RR
import rtamd as R
from anyhit_ref import LDS_ENTRIES
from test_gpu_trace_rays import _same

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
N_TWIN = 2000


def _need_gpu():
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _twin(scene):
    """The host twin's answers, once per scene: {(set, bound, k): (rays, tmax, (t, index, count))}."""
    c = S.ctx(scene)
    rng = np.random.default_rng(79)
    out = {}
    for name, rays in c["sets"].items():
        n = rays.shape[0] if (scene, name) == ("teapot", "random") else min(N_TWIN, rays.shape[0])
        r = np.ascontiguousarray(rays[:n])
        tm = S._tmax_classes(c["orc"].closest_hit(r)[0], rng)
        for b, tmax in (("none", None), ("classes", tm)):
            for k in S.KS:
                out[(name, b, k)] = (r, tmax, c["dev"].multi_hit(r, k, tmax))
    return out


def _assert_same(what, got, want, k):
    got = tuple(np.ascontiguousarray(g.cpu().numpy()) if isinstance(g, torch.Tensor) else g for g in got)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, g.dtype)
    bad = M.differing_rows(got, want, k)
    assert bad.size == 0, "%s: %d rows differ, first %d: gpu t %r index %r count %d, want t %r index %r count %d" % (
        what, bad.size, bad[0], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want[0][bad[0]], want[1][bad[0]],
        want[2][bad[0]])


def _assert_stats(what, q, counters, count, ctr):
    st = q.stats()
    n = count.shape[0]
    assert st["live_segments"] == n and st["hits"] == int((count >= 1).sum()), (what, st)
    assert st["misses"] == n - int((count >= 1).sum()) and st["hits_sphere"] == 0, (what, st)
    want = [int(v) for v in ctr.sum(0)] if counters else [0, 0, 0, 0]
    assert [st[x] for x in COUNTERS] == want, "%s: Pn/Iv/Tt/sphere tests: gpu %s yardstick %s" % (
        what, [st[x] for x in COUNTERS], want)


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", S.SCENES)
def test_equals_host_twin_and_yardstick(scene, counters):
    _need_gpu()
    torch.cuda.set_device(0)
    dev = S.ctx(scene)["dev"]
    q = R.RayQuery(dev, counters=counters)
    try:
        for (name, b, k), (rays, tmax, want) in _twin(scene).items():
            what = "%s/%s tmax=%s K=%d" % (scene, name, b, k)
            _assert_same(what + " numpy", q.multi_hit(rays, k, tmax), want, k)
            st = q.stats()
            assert st["live_segments"] == rays.shape[0] and st["hits"] == int((want[2] >= 1).sum()), what
            rays_t = torch.from_numpy(rays).cuda()
            got = q.multi_hit(rays_t, k, None if tmax is None else torch.from_numpy(tmax).cuda())
            assert all(g.device == rays_t.device for g in got)
            assert [g.dtype for g in got] == [torch.float32, torch.int32, torch.int32]
            _assert_same(what + " torch", got, want, k)
        for name, (rays, tm, res) in S.ref(scene).items():
            for b in S.BOUNDS:
                recs, count, ctr = res[b][:3]
                for k in S.KS:
                    what = "%s/%s tmax=%s K=%d yardstick" % (scene, name, b, k)
                    _assert_same(what, q.multi_hit(rays, k, None if b == "none" else tm), M.rows(recs, k) + (count,), k)
                    _assert_stats(what, q, counters, count, ctr)
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres", "twins"])
def test_batch_sizes(scene):
    _need_gpu()
    dev = S.ctx(scene)["dev"]
    name = "through" if scene == "twins" else "random"
    q = R.RayQuery(dev)
    try:
        for k in S.KS:
            rays_all, want = S.ctx(scene)["sets"][name], _twin(scene)[(name, "none", k)][2]
            for n in (0, 1, 63, 64, 65, 2037):
                rays = np.ascontiguousarray(rays_all[:n])
                got = q.multi_hit(rays, k)
                assert got[0].shape == (n, k) and got[1].shape == (n, k) and got[2].shape == (n,)
                if n <= want[2].shape[0]:
                    w = tuple(a[:n] for a in want)
                else:
                    w = dev.multi_hit(rays, k)
                _assert_same("%s n=%d K=%d" % (scene, n, k), got, w, k)
    finally:
        q.close()


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("name", ["axis_plus", "solid_plus", "tilted_plus", "interleaved"])
def test_deep_stack(name, k, counters):
    _need_gpu()
    rays, tm, res = S.deep(name, 1024)
    assert max(int(res[b][3].max()) for b in S.BOUNDS) > LDS_ENTRIES           # past the LDS entries
    if name == "solid_plus":
        assert int(res["none"][1].max()) == 60 > k                              # truncated rows
    q = R.RayQuery(S.ctx("deep")["dev"], counters=counters)
    try:
        for b in S.BOUNDS:
            recs, count, ctr = res[b][:3]
            what = "deep/%s K=%d tmax=%s" % (name, k, b)
            _assert_same(what, q.multi_hit(rays, k, None if b == "none" else tm), M.rows(recs, k) + (count,), k)
            _assert_stats(what, q, counters, count, ctr)
    finally:
        q.close()


def test_whole_grid():
    """2^20 rays = 4096 workgroups of 256 lanes, more than the library launches (CUs x resident workgroups per CU; see
    test_gpu_anyhit_order.test_whole_grid), so the grid is `blocks` and its last lanes address the end of the overflow
    buffer.  The rays are a fixed permutation of the 3072 interleaved deep rays, tiled."""
    _need_gpu()
    rays, tm, res = S.deep("interleaved", 1024)
    assert rays.shape[0] == 3072
    idx = np.random.default_rng(5).permutation(3072)[np.arange(1 << 20) % 3072]
    big = np.ascontiguousarray(rays[idx])
    for counters, k, b in ((True, 32, "none"), (False, 1, "classes")):
        recs, count, ctr = res[b][:3]
        t, index = M.rows(recs, k)
        q = R.RayQuery(S.ctx("deep")["dev"], counters=counters)
        try:
            got = q.multi_hit(big, k, None if b == "none" else np.ascontiguousarray(tm[idx]))
            what = "deep/whole grid K=%d tmax=%s" % (k, b)
            _assert_same(what, got, (t[idx], index[idx], count[idx]), k)
            _assert_stats(what, q, counters, count[idx], ctr[idx])
        finally:
            q.close()


def test_alternating_streams_and_update():
    """multi_hit, closest and occluded alternate on two torch streams on one object: they share the scratch and lay
    out the one overflow buffer differently.  Then the same after RayQuery.update, against the refitted host scene."""
    _need_gpu()
    torch.cuda.set_device(0)
    n, k = 1024, 8
    rays, tm, res = S.deep("interleaved", n)
    c = S.ctx("deep")
    dev = c["dev"]
    want_m = M.rows(res["classes"][0], k) + (res["classes"][1],)
    want_m0 = M.rows(res["none"][0], 64) + (res["none"][1],)
    t_c, i_c, _ = c["orc"].closest_hit(rays)
    rays_t, tm_t = torch.from_numpy(rays).cuda(), torch.from_numpy(tm).cuda()
    torch.cuda.synchronize()
    q = R.RayQuery(dev)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for _ in range(3):
            with torch.cuda.stream(s1):
                outs.append(("multi", q.multi_hit(rays_t, k, tm_t)))
            with torch.cuda.stream(s2):
                outs.append(("closest", q.closest(rays_t)))
            with torch.cuda.stream(s1):
                outs.append(("occluded", q.occluded(rays_t, tm_t)))
            with torch.cuda.stream(s2):
                outs.append(("multi0", q.multi_hit(rays_t, 64)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "multi":
                _assert_same("streams multi", r, want_m, k)
            elif kind == "multi0":
                _assert_same("streams multi0", r, want_m0, 64)
            elif kind == "closest":
                assert _same(t_c, i_c, r[0].cpu().numpy(), r[1].cpu().numpy()).size == 0
            else:
                assert np.array_equal(r.cpu().numpy(), res["classes"][1] >= 1)      # count >= 1 <=> occluded
    finally:
        q.close()
    for scene in ("teapot", "twins"):
        path, use_bvh = S.scene_path(scene)
        moved = R.Scene(path, use_bvh=use_bvh, image=S.IMG)
        V = RR.deform(moved.vertices(), "jitter")
        q = R.RayQuery(moved)                       # resident: the undeformed geometry
        moved.refit(V)                              # the host scene moves; q keeps its own copy until update
        try:
            r = np.ascontiguousarray(S.ctx(scene)["sets"]["random"][:N_TWIN])
            before = q.multi_hit(r, k)
            _assert_same("%s before update" % scene, before, S.ctx(scene)["dev"].multi_hit(r, k), k)
            q.update(V)
            want = moved.multi_hit(r, k)
            assert M.differing_rows(before, want, k).size > 0
            _assert_same("%s after update" % scene, q.multi_hit(r, k), want, k)
            _assert_same("%s after update, torch" % scene, q.multi_hit(torch.from_numpy(r).cuda(), k), want, k)
        finally:
            q.close()


def test_optional_outputs():
    """The raw _host call on pattern-filled buffers: an output whose pointer is NULL is not written, the others are
    exact (t alone and index alone keep the missing half of the list in the object's scratch), and with no output
    the call only traverses and counts."""
    _need_gpu()
    rays, tm, res = S.ref("twins")["through"]
    n, k = rays.shape[0], 8
    recs, count, ctr = res["classes"][:3]
    want = dict(zip(("t", "index", "count"), M.rows(recs, k) + (count,)))
    q = R.RayQuery(S.ctx("twins")["dev"], counters=True)
    f = q.L.rt_query_multi_hit_host
    f.argtypes = [R.P, R.P, R.P, R.I32, R.I32, R.P]
    try:
        for given in (("count",), ("t",), ("index",), (), ("t", "index", "count"), ("index", "count")):
            buf = {"t": np.full((n + 1, k), 7.5, np.float32), "index": np.full((n + 1, k), 77, np.int32),
                   "count": np.full(n + 1, 77, np.int32)}
            fill = {x: v.copy() for x, v in buf.items()}
            mo = R.RtMultiHitOut(**{x: R._ptr(buf[x]) for x in given})
            assert f(q.h, R._ptr(rays), R._ptr(tm), n, k, C.byref(mo)) == 0, q.L.rt_last_error()
            _assert_stats("outputs %s" % (given,), q, True, count, ctr)
            for x in ("t", "index", "count"):
                assert buf[x][n:].tobytes() == fill[x][n:].tobytes(), (given, x)
                if x in given:
                    assert (M.same(buf[x][:n], want[x]) if x == "t" else buf[x][:n] == want[x]).all(), (given, x)
                else:
                    assert buf[x].tobytes() == fill[x].tobytes(), (given, x)
    finally:
        q.close()
