"""Dynamic geometry on the GPU: rt_query_update_triangles / rtamd.RayQuery.update.

A RayQuery created from the ORIGINAL scene is updated with deformed vertices; then
  * geometry() -- the device's triangle records and node bounds -- equals rt_scene_refit of a second Scene,
    bitwise (the host twin, which tests/test_refit_host.py pins to the definition);
  * closest on 2000 rays per set is bit-exact (NaN = NaN) against rtamd.trace_rays on that host-refit Scene,
    the pre-existing one-shot upload path;
  * the first 300 rays per set are checked against refit_ref.ClosestRef (the reference traversal over the
    oracle's own intersection functions), with exact Pn/Iv/Tt/sphere-test sums under counters=True;
  * occluded on 300 rays per set, with test_gpu_query's bound classes, against AnyHitRef over the refit arrays.
Scenes: the smallest at which each code path can go wrong -- cornell, cornell no_bvh (root leaf: no records),
teapot (multi-workgroup levels and the chained top), deep (30 one-record levels: the chain launch alone),
big_leaf (the big_leaves table) and same-centroid scenes of 1, 5, 63, 64 and 65 triangles (root leaf, a split,
the inline-leaf limit).  Deformations: refit_ref.DEFORMATIONS.  A mismatch is diagnosed by reading the code.

The two Python yardsticks cost microseconds per traversal step, and teapot's 126,050 triangles under jitter,
translate_half and collapse give trees in which one ray takes 10^5 steps: all 300 rays per set took 85, 163 and 246 s
per case there.  So a yardstick stops taking further rays of a set once it has done WORK_BUDGET steps on it
(_within_budget; at least one ray): every other scene keeps all 300 (asserted), teapot keeps 1 to 300 per set depending
on the deformation, and the 2000 rays per set against the one-shot path are never cut.
"""
import atexit
import functools
import shutil
import tempfile

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import edge_scenes
import refit_ref as RR
import rtamd as R
from anyhit_ref import AnyHitRef
from test_gpu_query import _tmax_classes
from test_gpu_trace_rays import _ray_sets, _same

pytestmark = pytest.mark.gpu

IMG = (16, 16, 1, 1)
SCENES = ["cornell", "cornell:no_bvh", "teapot", "deep", "big_leaf", "same1", "same5", "same63", "same64", "same65"]
COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
N_CLOSEST, N_REF = 2000, 300
WORK_BUDGET = 60000   # yardstick steps per ray set (see _within_budget)


@functools.lru_cache(maxsize=None)
def _paths():
    d = tempfile.mkdtemp(prefix="refit_scenes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = dict(edge_scenes.write(d))
    for n in (1, 5, 63, 64, 65):
        out["same%d" % n] = "%s/same%d.scene" % (d, n)
        with open(out["same%d" % n], "w") as f:
            f.write(RR.same_centroid_scene(n))
    return out


def _load(scene):
    name, _, flag = scene.partition(":")
    path = _paths().get(name) or "%s/%s.scene" % (R.ASSETS, name)
    return R.Scene(path, use_bvh=flag != "no_bvh", image=IMG)


@functools.lru_cache(maxsize=None)
def _base(scene):
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    dev = _load(scene)
    return dict(dev=dev, V0=dev.vertices(), arrays=dev.arrays())


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_rows(what, got, want):
    rows = np.nonzero((_u32(got) != _u32(want)).any(axis=1))[0]
    assert rows.size == 0, "%s: %d rows differ, first %d: device %r host %r" % (
        what, rows.size, rows[0], got[rows[0]], want[rows[0]])


def _within_budget(query, n):
    """query(i) for i = 0, 1, ... < n until the yardstick has done WORK_BUDGET node pops, triangle and sphere tests
    (at least one ray).  The Python yardsticks cost microseconds per step; on every scene but teapot all n rays fit."""
    out, work = [], 0
    for i in range(n):
        out.append(query(i))
        work += sum(int(x) for x in out[-1][-4:]) - int(out[-1][-3])     # Pn + Tt + sphere tests (Iv is part of Pn)
        if work >= WORK_BUDGET:
            break
    return out


@functools.lru_cache(maxsize=None)
def _case(scene, deformation):
    """Per (scene, deformation), computed once: the vertices, the host-refit second Scene and its arrays, the
    ray sets over the deformed geometry and the yardsticks' answers on the first N_REF rays of each."""
    b = _base(scene)
    W = RR.deform(b["V0"], deformation)
    host = _load(scene)
    host.refit(W)
    arr = host.arrays()
    finite = np.isfinite(arr["triangles"][:, 0:9]).all(axis=1)    # ray origins from the finite vertices (a zero-area
                                                                 # triangle has a NaN normal)
    sets = _ray_sets(RR.Arrays(arr, triangles=arr["triangles"][finite]), np.random.default_rng(1234), N_CLOSEST)
    shim = RR.Arrays(arr)
    cref, aref = RR.ClosestRef(shim), AnyHitRef(shim)
    rng = np.random.default_rng(77)
    ref = {}
    for k, rays in sets.items():
        r = np.ascontiguousarray(rays[:N_REF])
        res = _within_budget(lambda i: cref.query(r[i]), N_REF)
        t = np.array([x[0] for x in res], np.float32)
        idx = np.array([x[1] for x in res], np.int32)
        ctr = np.array([x[2:] for x in res], np.int64)
        tm = _tmax_classes(t, rng)
        m0 = np.array([x[0] for x in _within_budget(lambda i: aref.query(r[i], None), len(res))], np.bool_)
        m1 = np.array([x[0] for x in _within_budget(lambda i: aref.query(r[i], tm[i]), len(res))], np.bool_)
        ref[k] = (r, t, idx, ctr, tm, m0, m1)
    return dict(W=W, host=host, arr=arr, sets=sets, ref=ref)


@pytest.mark.parametrize("deformation", RR.DEFORMATIONS)
@pytest.mark.parametrize("scene", SCENES)
def test_update_then_geometry_and_queries(scene, deformation):
    b, c = _base(scene), _case(scene, deformation)
    q, qc = R.RayQuery(b["dev"]), R.RayQuery(b["dev"], counters=True)
    try:
        q.update(c["W"])
        qc.update(c["W"])
        assert all(v == 0 for k, v in q.stats().items()), "stats after an update, no query since"
        for obj in (q, qc):
            tri, bvh = obj.geometry()
            _assert_rows("%s/%s triangles" % (scene, deformation), tri, c["arr"]["triangles"])
            _assert_rows("%s/%s nodes" % (scene, deformation), bvh, c["arr"]["bvh"])
        names = list(c["sets"])
        rays = np.ascontiguousarray(np.concatenate([c["sets"][k] for k in names]))
        t_h, i_h, _ = R.trace_rays(c["host"], rays)             # one-shot upload of the host-refit scene
        t_g, i_g = q.closest(rays)
        bad = _same(t_h, i_h, t_g, i_g)
        assert bad.size == 0, "%s/%s closest: %d rays differ, first %d (set %s): host-refit (%r, %d) updated (%r, %d)" % (
            scene, deformation, bad.size, bad[0], names[bad[0] // N_CLOSEST], t_h[bad[0]], i_h[bad[0]], t_g[bad[0]],
            i_g[bad[0]])
        for k, (r, t, idx, ctr, tm, m0, m1) in c["ref"].items():
            n = t.shape[0]                                          # N_REF unless the yardstick's budget cut it
            t_g, i_g = qc.closest(np.ascontiguousarray(r[:n]))
            bad = _same(t, idx, t_g, i_g)
            assert bad.size == 0, "%s/%s/%s: %d rays differ from ClosestRef, first %d: ref (%r, %d) gpu (%r, %d)" % (
                scene, deformation, k, bad.size, bad[0], t[bad[0]], idx[bad[0]], t_g[bad[0]], i_g[bad[0]])
            st = qc.stats()
            assert [st[x] for x in COUNTERS] == [int(v) for v in ctr.sum(0)], (scene, deformation, k)
            assert st["live_segments"] == n and st["hits"] == int((idx >= 0).sum())
            assert scene == "teapot" or n == N_REF
            for what, tmax, want in (("None", None, m0), ("classes", tm, m1)):
                m = want.shape[0]
                got = q.occluded(np.ascontiguousarray(r[:m]), None if tmax is None else np.ascontiguousarray(tmax[:m]))
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, "%s/%s/%s occluded tmax=%s: %d rays differ, first %d (class %d): ref %d gpu %d" % (
                    scene, deformation, k, what, bad.size, bad[0], bad[0] % 11, want[bad[0]], got[bad[0]])
    finally:
        q.close()
        qc.close()


def _all_rays(c):
    return np.ascontiguousarray(np.concatenate([v[:N_REF] for v in c["sets"].values()]))


@pytest.mark.parametrize("scene", ["teapot", "cornell:no_bvh"])
def test_sequence_returns_to_the_first_state(scene):
    b = _base(scene)
    A, B = _case(scene, "jitter"), _case(scene, "translate_half")
    rays = _all_rays(_case(scene, "identity"))
    q = R.RayQuery(b["dev"])
    try:
        q.update(b["V0"])
        first, geo_first = q.closest(rays), q.geometry()
        for c in (A, B):
            q.update(c["W"])
            t_h, i_h, _ = R.trace_rays(c["host"], rays)
            t_g, i_g = q.closest(rays)
            assert _same(t_h, i_h, t_g, i_g).size == 0
            _assert_rows("nodes", q.geometry()[1], c["arr"]["bvh"])
        assert _same(first[0], first[1], *q.closest(rays)).size > 0       # B's geometry gives other answers
        q.update(b["V0"])
        last, geo_last = q.closest(rays), q.geometry()
        assert _same(first[0], first[1], last[0], last[1]).size == 0
        _assert_rows("triangles", geo_last[0], geo_first[0])
        _assert_rows("nodes", geo_last[1], geo_first[1])
    finally:
        q.close()


def test_torch_streams():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    torch.cuda.set_device(0)
    b = _base("teapot")
    A, B = _case("teapot", "jitter"), _case("teapot", "translate_half")
    rays = _all_rays(A)
    q = R.RayQuery(b["dev"])
    try:
        want = {}
        for name, c in (("A", A), ("B", B)):                    # the blocking path
            q.update(c["W"])
            want[name] = q.closest(rays)
        assert _same(*want["A"], *want["B"]).size > 0
        rays_t = torch.from_numpy(rays).cuda()
        half = torch.from_numpy(np.ascontiguousarray(A["W"] * np.float32(0.5))).cuda()
        WB = torch.from_numpy(B["W"]).cuda()
        q.reserve(rays.shape[0])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                           # update then closest, back to back, no sync
            WA = half + half                                    # produced on `side`, read in stream order
            q.update(WA)
            t1, i1 = q.closest(rays_t)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):                             # update on one stream ...
            q.update(WB)
        with torch.cuda.stream(s2):                             # ... closest on another: the event chain orders them
            t2, i2 = q.closest(rays_t)
        with torch.cuda.stream(s1):
            q.update(WA)
        with torch.cuda.stream(side):
            t3, i3 = q.closest(rays_t)
        torch.cuda.synchronize()
        assert np.array_equal(WA.cpu().numpy().view(np.uint32), A["W"].view(np.uint32))
        assert _same(*want["A"], t1.cpu().numpy(), i1.cpu().numpy()).size == 0
        assert _same(*want["B"], t2.cpu().numpy(), i2.cpu().numpy()).size == 0
        assert _same(*want["A"], t3.cpu().numpy(), i3.cpu().numpy()).size == 0
        _assert_rows("nodes", q.geometry()[1], A["arr"]["bvh"])
    finally:
        q.close()


def test_wrong_inputs_are_refused_and_change_nothing():
    b = _base("cornell")
    V = b["V0"]
    q = R.RayQuery(b["dev"])
    try:
        before = q.geometry()
        Vt = torch.from_numpy(V).cuda()
        for x in (V.astype(np.float64), V[:, :8], V.reshape(-1), np.zeros((V.shape[0], 18), np.float32)[:, ::2],
                  Vt.double(), Vt[:, :6], Vt.t().contiguous().t(), Vt.cpu(), Vt.reshape(-1)):
            with pytest.raises(ValueError):
                q.update(x)
        for x in (np.ascontiguousarray(V[:-1]), Vt[:-1].contiguous()):
            with pytest.raises(R.RtError, match="triangle_count"):
                q.update(x)
        after = q.geometry()
        _assert_rows("triangles", after[0], before[0])
        _assert_rows("nodes", after[1], before[1])
        _assert_rows("triangles", before[0], b["arrays"]["triangles"])       # and a fresh object holds the scene's
        _assert_rows("nodes", before[1], b["arrays"]["bvh"])
    finally:
        q.close()


def test_updates_allocate_nothing_after_the_first():
    torch.cuda.set_device(0)
    b = _base("teapot")
    A, B = _case("teapot", "jitter"), _case("teapot", "translate_half")
    rays = _all_rays(A)
    q = R.RayQuery(b["dev"])
    try:
        WA, WB = torch.from_numpy(A["W"]).cuda(), torch.from_numpy(B["W"]).cuda()
        rays_t = torch.from_numpy(rays).cuda()
        q.update(WA)
        q.update(A["W"])                                        # the host path's staging, once
        q.reserve(rays.shape[0])
        want = {}
        for name, W in (("A", WA), ("B", WB)):
            q.update(W)
            t, i = q.closest(rays_t)                            # also warms torch's allocator for the outputs
            want[name] = (t.cpu().numpy(), i.cpu().numpy())
            del t, i
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        for k in range(10):
            name, W = (("A", WA), ("B", WB))[k % 2]
            q.update(W if k % 4 < 2 else W.cpu().numpy())
            t, i = q.closest(rays_t)
            assert _same(*want[name], t.cpu().numpy(), i.cpu().numpy()).size == 0, k
            del t, i
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free0
    finally:
        q.close()
