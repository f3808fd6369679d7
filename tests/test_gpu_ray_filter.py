"""Filtered ray queries on the GPU: rt_query_closest_filtered and rt_query_occluded_filtered (rtamd.RayQuery)
against their host twins and against the yardstick (tests/ray_filter_ref.py).

* every output of every row equals the twin bit for bit on numpy input and on torch tensors with tensor filter members
  (2,000 rays per set, the 300 filter classes of tests/ray_filter_scenes.py repeated), and the yardstick on the first
  300 (16 on teapot); with the counters build and without; with counters on, the summed Pn, Iv, Tt and sphere tests
  equal the twin's and the yardstick's to the unit, and stats() is as specified;
* batch sizes around the wave and workgroup size;
* deep's constructed sets, whose stacks pass the LDS entries into the overflow buffer, interleaved with shallow rays in
  one wave, for both kernels; one 2^20-ray call;
* closest_filtered, closest, occluded and nearest_k alternating on two streams (one scratch, one overflow buffer);
  set_masks between calls on different streams, then dropped; after update; constant free device memory over ten
  rounds; fields=() only traverses.
The twin's and the yardstick's answers are computed once per process and shared.
"""
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import edge_scenes
import multihit_scenes as M
import ray_filter_ref as RF
import ray_filter_scenes as FS
import refit_ref as RR
import rtamd as R

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
N_SET = 2000


def _need_gpu():
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_t(a, b):
    """Equal bit for bit, a NaN being any NaN (rt_abi.h)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _cuda_members(f):
    """Tensor filter members; the uint32 ray masks as int32 tensors of the same bits."""
    return {k: (None if v is None else _cuda(v.view(np.int32) if v.dtype == np.uint32 else v)) for k, v in f.items()}


def _np(v):
    return np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v


@functools.lru_cache(maxsize=None)
def _twin(scene, name, run):
    """The host twin over the set's first N_SET rays under the run's classes, repeated:
    (rays, members, masks, hit records dict, closest stats, occluded, any-hit stats)."""
    c = M.ctx(scene)
    rays = np.ascontiguousarray(c["sets"][name][:N_SET])
    f = FS.filters(scene, name, FS.n_ref(scene))[run]
    fm = FS.tiled(f, rays.shape[0])
    rec, st = c["dev"].closest_filtered(rays, masks=f["masks"], fields=R.HIT_FIELDS, stats=True, **fm)
    occ, sta = c["dev"].occluded_filtered(rays, masks=f["masks"], stats=True, **fm)
    return rays, fm, f["masks"], rec, st, occ, sta


def _same_records(what, got, want, fields):
    assert tuple(got) == tuple(fields), (what, tuple(got))
    for k in fields:
        g, w = _np(got[k]), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        if g.shape[0] == 0:
            continue
        bad =np.nonzero((g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)).any(1))[0]
        # a NaN is any NaN (rt_abi.h): rows whose floats differ only in NaN payloads are equal
        if bad.size and g.dtype == np.float32:
            bad = bad[[not np.array_equal(g[i], w[i], equal_nan=True) for i in bad]]
        assert bad.size == 0, "%s: %s differs in %d rows, first %d: gpu %r want %r" % (what, k, bad.size, bad[0], g[bad[0]], w[bad[0]])


def _stats(what, q, n, hits, hits_sphere=None, ctr=None):
    st = q.stats()
    assert st["live_segments"] == n and st["hits"] == hits and st["misses"] == n - hits, (what, st)
    if hits_sphere is not None:
        assert st["hits_sphere"] == hits_sphere, (what, st)
    if ctr is not None:
        assert [st[k] for k in COUNTERS] == [int(v) for v in ctr], "%s: Pn/Iv/Tt/sphere tests: gpu %s want %s" % (
            what, [st[k] for k in COUNTERS], list(ctr))


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", FS.SCENES)
def test_equals_host_twin_and_yardstick(scene, counters):
    _need_gpu()
    torch.cuda.set_device(0)
    dev = M.ctx(scene)["dev"]
    S = dev.view.sphere_count
    q = R.RayQuery(dev, counters=counters)
    zero = [0, 0, 0, 0]
    try:
        for name in M.ctx(scene)["sets"]:
            for k, run in enumerate(FS.RUNS):
                rays, fm, masks, rec, st, occ, sta = _twin(scene, name, run)
                n = rays.shape[0]
                what = "%s/%s/%s" % (scene, name, run)
                # the masks through the host call and through a tensor in turn
                q.set_masks(masks if masks is None or k % 2 else _cuda(masks.view(np.int32)))
                fields = R.HIT_FIELDS if run == "all" else ("t", "index")
                want_c = [st[x] for x in COUNTERS] if counters else zero
                want_a = [sta[x] for x in COUNTERS] if counters else zero
                _same_records(what + " numpy", q.closest_filtered(rays, fields=fields, **fm), rec, fields)
                _stats(what, q, n, st["hits"], st["hits_sphere"], want_c)
                got = q.closest_filtered(_cuda(rays), fields=fields, **_cuda_members(fm))
                assert all(g.is_cuda and g.is_contiguous() for g in got.values())
                _same_records(what + " torch", got, rec, fields)
                _stats(what + " torch", q, n, st["hits"], st["hits_sphere"], want_c)
                assert np.array_equal(q.occluded_filtered(rays, **fm), occ), what
                _stats(what + " any-hit", q, n, sta["hits"], None, want_a)
                got = q.occluded_filtered(_cuda(rays), **_cuda_members(fm))
                assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), occ), what
                _stats(what + " any-hit torch", q, n, sta["hits"], None, want_a)
                # the yardstick on the rows it answered
                e = FS.ref(scene)[name][run]
                m = e["rays"].shape[0]
                f1 = FS.members(e["filter"])
                got = q.closest_filtered(e["rays"], **f1)
                assert same_t(got["t"], e["closest"][0]) and np.array_equal(got["index"], e["closest"][1]), what
                hs = int(((e["closest"][1] >= 0) & (e["closest"][1] < S)).sum())
                _stats(what + " yardstick", q, m, int((e["closest"][1] >= 0).sum()), hs, e["closest"][2].sum(0) if counters else zero)
                assert np.array_equal(q.occluded_filtered(e["rays"], **f1), e["anyhit"][0]), what
                _stats(what + " yardstick any-hit", q, m, int(e["anyhit"][0].sum()), None, e["anyhit"][1].sum(0) if counters else zero)
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres", "twins"])
def test_batch_sizes(scene):
    _need_gpu()
    name = "through" if scene == "twins" else "random"
    rays_all, fm_all, masks, rec, _, occ, _ = _twin(scene, name, "all")
    q = R.RayQuery(M.ctx(scene)["dev"])
    try:
        q.set_masks(masks)
        for n in (0, 1, 63, 64, 65, 2037):
            rep = np.arange(n) % rays_all.shape[0]
            rays = np.ascontiguousarray(rays_all[rep])
            fm = {k: np.ascontiguousarray(v[rep]) for k, v in fm_all.items()}
            want = {k: rec[k][rep] for k in ("t", "index")}
            got = q.closest_filtered(rays, **fm)
            assert got["t"].shape == (n,) and got["index"].shape == (n,)
            _same_records("%s n=%d" % (scene, n), got, want, ("t", "index"))
            _same_records("%s n=%d torch" % (scene, n), q.closest_filtered(_cuda(rays), **_cuda_members(fm)), want, ("t", "index"))
            assert np.array_equal(q.occluded_filtered(rays, **fm), occ[rep])
            assert np.array_equal(q.occluded_filtered(_cuda(rays), **_cuda_members(fm)).cpu().numpy(), occ[rep])
    finally:
        q.close()


@functools.lru_cache(maxsize=None)
def _deep_weave():
    """deep's three constructed sets, 1,024 rays each, interleaved ray by ray, so every wave holds rays whose stacks
    pass the LDS entries (axis_plus, solid_plus) beside shallow ones; the filter skips the primitive the unfiltered
    walk found, so stopped rays go on behind it, and bounds the interval on every third ray.
    -> (rays, members, twin t, twin index, twin occluded)."""
    dev = M.ctx("deep")["dev"]
    rays = edge_scenes.interleaved(edge_scenes.axis_plus(1024), edge_scenes.solid_plus(1024), edge_scenes.tilted_plus(1024))
    first = dev.closest_filtered(rays)
    n = rays.shape[0]
    tmin = np.where(np.arange(n) % 3 == 0, np.float32(2.0), np.float32(0)).astype(np.float32)
    fm = dict(tmin=tmin, tmax=np.full(n, 1e28, np.float32), skip=np.ascontiguousarray(first["index"]),
              mask=np.full(n, 0xFFFFFFFF, np.uint32))
    got = dev.closest_filtered(rays, **fm)
    return rays, fm, got["t"], got["index"], dev.occluded_filtered(rays, **fm)


@pytest.mark.parametrize("counters", [True, False])
def test_deep_stacks_interleaved_with_shallow_rays(counters):
    _need_gpu()
    r = FS.ref("deep")
    assert int(r["axis_plus"]["none"]["closest"][3][:, 0].max()) > RF.CLOSEST_LDS       # past the LDS pairs
    assert int(r["axis_plus"]["none"]["closest"][3][:, 1].max()) > 0                     # and popped from there
    assert int(r["axis_plus"]["none"]["anyhit"][2][:, 0].max()) > RF.ANYHIT_LDS
    rays, fm, t, idx, occ = _deep_weave()
    assert (idx >= 0).any() and (idx < 0).any()
    q = R.RayQuery(M.ctx("deep")["dev"], counters=counters)
    try:
        for _ in range(2):
            got = q.closest_filtered(rays, **fm)
            assert same_t(got["t"], t) and np.array_equal(got["index"], idx)
            assert np.array_equal(q.occluded_filtered(_cuda(rays), **_cuda_members(fm)).cpu().numpy(), occ)
    finally:
        q.close()


def test_whole_grid():
    """2^20 rays = 4096 workgroups of 256 lanes, more than the library launches, so the grid is `blocks` and its last
    lanes address the end of the overflow buffer: a fixed permutation of deep's interleaved rays, tiled."""
    _need_gpu()
    rays, fm, t, idx, occ = _deep_weave()
    pick = np.random.default_rng(5).permutation(rays.shape[0])[np.arange(1 << 20) % rays.shape[0]]
    big = np.ascontiguousarray(rays[pick])
    fb = {k: np.ascontiguousarray(v[pick]) for k, v in fm.items()}
    for counters in (True, False):
        q = R.RayQuery(M.ctx("deep")["dev"], counters=counters)
        try:
            got = q.closest_filtered(big, **fb)
            assert same_t(got["t"], t[pick]) and np.array_equal(got["index"], idx[pick])
            _stats("whole grid", q, 1 << 20, int((idx[pick] >= 0).sum()))
            assert np.array_equal(q.occluded_filtered(big, **fb), occ[pick])
            _stats("whole grid any-hit", q, 1 << 20, int(occ[pick].sum()))
        finally:
            q.close()


def test_alternating_streams():
    """closest_filtered, closest, occluded and nearest_k alternate on two torch streams on one object: they share the
    slots, the queue words and the one overflow buffer (the other queries' own answers come from a second object, one
    call at a time)."""
    _need_gpu()
    torch.cuda.set_device(0)
    dev = M.ctx("deep")["dev"]
    rays, fm, t, idx, occ_f = _deep_weave()
    pts = np.ascontiguousarray(rays[:, :3] + rays[:, 3:6])
    q0 = R.RayQuery(dev)
    try:
        ct, ci = q0.closest(rays)
        occ = q0.occluded(rays)
        near = q0.nearest_k(pts, 4)
    finally:
        q0.close()
    torch.cuda.synchronize()
    rays_t, fm_t, pts_t = _cuda(rays), _cuda_members(fm), _cuda(pts)
    q = R.RayQuery(dev)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for _ in range(3):
            with torch.cuda.stream(s1):
                outs.append(("filtered", q.closest_filtered(rays_t, **fm_t)))
            with torch.cuda.stream(s2):
                outs.append(("closest", q.closest(rays_t)))
            with torch.cuda.stream(s1):
                outs.append(("occluded", q.occluded(rays_t)))
            with torch.cuda.stream(s2):
                outs.append(("any", q.occluded_filtered(rays_t, **fm_t)))
            with torch.cuda.stream(s1):
                outs.append(("nearest", q.nearest_k(pts_t, 4)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "filtered":
                assert same_t(_np(r["t"]), t) and np.array_equal(_np(r["index"]), idx)
            elif kind == "closest":
                assert same_t(_np(r[0]), ct) and np.array_equal(_np(r[1]), ci)
            elif kind == "occluded":
                assert np.array_equal(_np(r), occ)
            elif kind == "any":
                assert np.array_equal(_np(r), occ_f)
            else:
                for k in ("distance", "index", "count"):
                    assert np.array_equal(_np(r[k]).view(np.uint8), near[k].view(np.uint8)), k
    finally:
        q.close()


def test_set_masks_between_calls_on_two_streams():
    """set_masks joins the event chain: a call enqueued before it sees the old masks, one after it the new, whatever
    the streams; None drops them again."""
    _need_gpu()
    torch.cuda.set_device(0)
    scene = "cornell_plus"
    dev = M.ctx(scene)["dev"]
    rays, fm, masks, rec, _, occ, _ = _twin(scene, "random", "mask")
    other = np.ascontiguousarray(~masks)
    want_other = dev.closest_filtered(rays, masks=other, **fm)
    want_none = dev.closest_filtered(rays, **fm)
    assert not np.array_equal(want_other["index"], rec["index"]) and not np.array_equal(want_none["index"], rec["index"])
    rays_t, fm_t = _cuda(rays), _cuda_members(fm)
    m1, m2 = _cuda(masks.view(np.int32)), _cuda(other.view(np.int32))
    q = R.RayQuery(dev)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        torch.cuda.synchronize()
        for _ in range(3):
            with torch.cuda.stream(s1):
                q.set_masks(m1)
            with torch.cuda.stream(s2):
                outs.append((q.closest_filtered(rays_t, **fm_t), rec))
            with torch.cuda.stream(s1):
                q.set_masks(m2)
                outs.append((q.closest_filtered(rays_t, **fm_t), want_other))
            with torch.cuda.stream(s2):
                outs.append((q.occluded_filtered(rays_t, **fm_t), want_other["index"] >= 0))
        s1.synchronize()
        s2.synchronize()
        for got, want in outs:
            if isinstance(got, dict):
                _same_records("set_masks", got, want, ("t", "index"))
            else:
                assert np.array_equal(_np(got), want)
        assert q.stats()["live_segments"] == rays.shape[0]
        q.set_masks(m1)
        assert q.stats()["live_segments"] == 0              # like an update: nothing was traced since
        q.set_masks(None)
        _same_records("masks dropped", q.closest_filtered(rays, **fm), want_none, ("t", "index"))
        with pytest.raises(R.RtError, match="count"):
            q.L.rt_query_set_masks_host.argtypes = [R.P, R.P, R.I32]
            R._check(q.L.rt_query_set_masks_host(q.h, R._ptr(masks), masks.shape[0] - 1), q.L)
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "twins"])
def test_after_update_the_masks_survive(scene):
    _need_gpu()
    torch.cuda.set_device(0)
    path, use_bvh = M.scene_path(scene)
    moved = R.Scene(path, use_bvh=use_bvh, image=M.IMG)
    V = RR.deform(moved.vertices(), "jitter")
    name = "through" if scene == "twins" else "random"
    rays, fm, masks, rec, _, occ, _ = _twin(scene, name, "all")
    q = R.RayQuery(moved)                           # resident: the undeformed geometry
    moved.refit(V)                                  # the host scene moves; q keeps its own copy until update
    try:
        q.set_masks(masks)
        _same_records("%s before update" % scene, q.closest_filtered(rays, fields=R.HIT_FIELDS, **fm), rec, R.HIT_FIELDS)
        q.update(_cuda(V))
        new = moved.closest_filtered(rays, masks=masks, fields=R.HIT_FIELDS, **fm)
        assert not same_t(new["t"], rec["t"])
        _same_records("%s after update" % scene, q.closest_filtered(rays, fields=R.HIT_FIELDS, **fm), new, R.HIT_FIELDS)
        got = q.closest_filtered(_cuda(rays), fields=R.HIT_FIELDS, **_cuda_members(fm))
        _same_records("%s after update, torch" % scene, got, new, R.HIT_FIELDS)
        assert np.array_equal(q.occluded_filtered(rays, **fm), moved.occluded_filtered(rays, masks=masks, **fm))
    finally:
        q.close()


def test_constant_free_memory_and_traverse_only():
    """Once the scratch holds n rays the device-pointer calls allocate nothing: free device memory is the same after
    ten rounds of every call; fields=() writes nothing, returns nothing and counts."""
    _need_gpu()
    torch.cuda.set_device(0)
    scene = "cornell_plus"
    rays, fm, masks, rec, st, occ, _ = _twin(scene, "random", "all")
    rays_t, fm_t, masks_t = _cuda(rays), _cuda_members(fm), _cuda(masks.view(np.int32))
    q = R.RayQuery(M.ctx(scene)["dev"], counters=True)
    try:
        q.reserve(rays.shape[0])
        q.set_masks(masks_t)
        out = {k: torch.empty((rays.shape[0],) + R.HIT_SHAPES[k][0], dtype={np.float32: torch.float32, np.int32: torch.int32,
                                                                          np.uint8: torch.bool}[R.HIT_SHAPES[k][1]],
                              device="cuda") for k in R.HIT_FIELDS}
        o8 = torch.empty(rays.shape[0], dtype=torch.bool, device="cuda")
        ho = R.RtHitOut(**{k: v.data_ptr() for k, v in out.items()})
        rf = R.RtRayFilter(**{k: v.data_ptr() for k, v in fm_t.items()})
        L = q.L
        L.rt_query_closest_filtered.argtypes = [R.P, R.P, R.P, R.I32, R.P, R.P]
        L.rt_query_occluded_filtered.argtypes = [R.P, R.P, R.P, R.I32, R.P, R.P]
        L.rt_query_set_masks.argtypes = [R.P, R.P, R.I32, R.P]
        import ctypes as C

        def round_():
            n = rays.shape[0]
            assert L.rt_query_set_masks(q.h, R.P(masks_t.data_ptr()), masks.shape[0], None) == 0
            assert L.rt_query_closest_filtered(q.h, R.P(rays_t.data_ptr()), C.byref(rf), n, C.byref(ho), None) == 0
            assert L.rt_query_occluded_filtered(q.h, R.P(rays_t.data_ptr()), C.byref(rf), n, R.P(o8.data_ptr()), None) == 0
        round_()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(10):
            round_()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
        _same_records("raw call", out, rec, R.HIT_FIELDS)
        assert np.array_equal(o8.cpu().numpy(), occ)
        assert q.closest_filtered(rays_t, fields=(), **fm_t) == {}
        _stats("fields=()", q, rays.shape[0], st["hits"], st["hits_sphere"], [st[x] for x in COUNTERS])
        assert q.closest_filtered(rays, fields=(), **fm) == {}
        _stats("fields=() numpy", q, rays.shape[0], st["hits"], st["hits_sphere"], [st[x] for x in COUNTERS])
    finally:
        q.close()
