"""Hemisphere visibility queries on the GPU: rt_query_hemisphere (rtamd.RayQuery.hemisphere) against its host
twin and against the yardstick (tests/hemisphere_ref.py).

* every row equals the twin on numpy input and on torch tensors, for n in {0, 1, 63, 257} and S in {1, 3, 64, 65, 200} (a
  wave holds several points, a point spans waves and workgroups, n * S is no multiple of 64 and lies on either side of
  the smallest queue chunk), for n = 1 with S = 4096 (every atomic on one address), both modes, every filter class of
  tests/hemisphere_scenes.py with masks set; the yardstick on the first 300 work items (16 on teapot);
* counters and stats() to the unit, with the counters build and without;
* the deep frames (hemisphere_scenes: they stay inside the LDS entries) interleaved with shallow ones; the same call
  twice; hemisphere, occluded_filtered and closest alternating on two streams; after update and after set_masks;
  constant free device memory over ten rounds; one call with n * S = 2^20.
The twin's and the yardstick's answers are computed once per process and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import hemisphere_scenes as HS
import multihit_scenes as M
import refit_ref as RR
import rtamd as R

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
FIELDS = ("open_count", "openness")
N_ROWS = 257
SAMPLES = (3, 64, 65, 200, 1)


def _need_gpu():
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")


def _cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _cuda_members(f):
    """Tensor filter members; the uint32 ray masks as int32 tensors of the same bits."""
    return {k: (None if v is None else _cuda(v.view(np.int32) if v.dtype == np.uint32 else v)) for k, v in f.items()}


def _np(v):
    return np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v


def _same(what, got, want):
    assert tuple(got) == FIELDS, (what, tuple(got))
    for k in FIELDS:
        g, w = _np(got[k]), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, g.dtype)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, "%s: %s differs in %d rows, first %d: gpu %r want %r" % (what, k, bad.size, bad[0], g[bad[0]], w[bad[0]])


def _stats(what, q, st, counters):
    got = q.stats()
    assert got["live_segments"] == st["live_segments"] and got["hits"] == st["hits"] and got["misses"] == st["misses"], (what, got)
    want = [st[k] for k in COUNTERS] if counters else [0, 0, 0, 0]
    assert [got[k] for k in COUNTERS] == want, "%s: Pn/Iv/Tt/sphere tests: gpu %s want %s" % (what, [got[k] for k in COUNTERS], want)


@functools.lru_cache(maxsize=None)
def _twin(scene, name, run, samples, mode, rows=N_ROWS):
    """The host twin over `rows` frames of the set (its 300 frame and filter classes repeated):
    (points, normals, members, masks, the twin's fields, its stats)."""
    pts, nrm, _ = HS.frames(scene, name)
    f = HS.filters(scene, name)[run]
    pts, nrm = HS.tiled(pts, rows), HS.tiled(nrm, rows)
    fm = {k: HS.tiled(f[k], rows) for k in HS.MEMBERS}
    out, st = M.ctx(scene)["dev"].hemisphere(pts, nrm, samples, mode, seed=21, point_offset=7, masks=f["masks"], stats=True, **fm)
    return pts, nrm, fm, f["masks"], out, st


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", HS.SCENES)
def test_equals_host_twin_and_yardstick(scene, counters):
    _need_gpu()
    torch.cuda.set_device(0)
    dev = M.ctx(scene)["dev"]
    q = R.RayQuery(dev, counters=counters)
    rows = 33 if scene == "teapot" else N_ROWS
    try:
        case = 0
        for name in M.ctx(scene)["sets"]:
            for run in HS.RUNS:
                case += 1
                S, mode = SAMPLES[case % len(SAMPLES)], ("cosine", "uniform")[(case // len(SAMPLES)) % 2]
                pts, nrm, fm, masks, want, st = _twin(scene, name, run, S, mode, rows)
                what = "%s/%s/%s S=%d %s" % (scene, name, run, S, mode)
                # the masks through the host call and through a tensor in turn
                q.set_masks(masks if masks is None or case % 2 else _cuda(masks.view(np.int32)))
                _same(what + " numpy", q.hemisphere(pts, nrm, S, mode, seed=21, point_offset=7, **fm), want)
                _stats(what, q, st, counters)
                got = q.hemisphere(_cuda(pts), _cuda(nrm), S, mode, seed=21, point_offset=7, **_cuda_members(fm))
                assert all(g.is_cuda and g.is_contiguous() for g in got.values())
                assert got["open_count"].dtype == torch.int32 and got["openness"].dtype == torch.float32
                _same(what + " torch", got, want)
                _stats(what + " torch", q, st, counters)
                # the yardstick on the work items it walked
                for ymode, (yp, yn, yfm, ymasks, yS, res) in HS.ref(scene)[name][run].items():
                    got = q.hemisphere(yp, yn, yS, ymode, seed=11, **yfm)
                    assert np.array_equal(got["open_count"], res["open_count"]), what + " yardstick " + ymode
                    nopen = int(res["open_count"].sum())
                    yst = dict(zip(COUNTERS, (int(v) for v in res["counters"])), live_segments=yp.shape[0] * yS,
                               hits=yp.shape[0] * yS - nopen, misses=nopen)
                    _stats(what + " yardstick " + ymode, q, yst, counters)
    finally:
        q.close()


@pytest.mark.parametrize("samples", [1, 3, 64, 65, 200])
def test_batch_sizes(samples):
    """n * S from 1 to 51,400: below a wave, below and above the smallest queue chunk (64), no multiple of 64."""
    _need_gpu()
    scene = "cornell_plus"
    mode = "uniform" if samples in (3, 65) else "cosine"
    pts_all, nrm_all, fm_all, masks, want_all, _ = _twin(scene, "random", "all", samples, mode)
    dev = M.ctx(scene)["dev"]
    q = R.RayQuery(dev)
    try:
        q.set_masks(masks)
        for n in (0, 1, 63, 257):
            pts, nrm = pts_all[:n], nrm_all[:n]
            fm = {k: np.ascontiguousarray(v[:n]) for k, v in fm_all.items()}
            want = {k: want_all[k][:n] for k in FIELDS}          # point_offset makes a prefix the batch's own rows
            got = q.hemisphere(pts, nrm, samples, mode, seed=21, point_offset=7, **fm)
            assert got["open_count"].shape == (n,) and got["openness"].shape == (n,)
            _same("n=%d S=%d" % (n, samples), got, want)
            _same("n=%d S=%d torch" % (n, samples),
                  q.hemisphere(_cuda(pts), _cuda(nrm), samples, mode, seed=21, point_offset=7, **_cuda_members(fm)), want)
            # each output alone
            for k in FIELDS:
                one = q.hemisphere(pts, nrm, samples, mode, seed=21, point_offset=7, fields=k, **fm)
                assert list(one) == [k] and np.array_equal(one[k].view(np.uint32), want[k].view(np.uint32))
    finally:
        q.close()


@pytest.mark.parametrize("counters", [True, False])
def test_one_point_4096_samples(counters):
    """n = 1, S = 4096: every lane of every wave adds to the same count."""
    _need_gpu()
    scene = "cornell_plus"
    dev = M.ctx(scene)["dev"]
    pts, nrm, skip = HS.frames(scene, "random")
    q = R.RayQuery(dev, counters=counters)
    try:
        for row in (0, 1, 2):
            p, nm, sk = pts[row:row + 1], nrm[row:row + 1], np.ascontiguousarray(skip[row:row + 1])
            for mode in ("cosine", "uniform"):
                want, st = dev.hemisphere(p, nm, 4096, mode, seed=row, skip=sk, stats=True)
                _same("row %d %s" % (row, mode), q.hemisphere(p, nm, 4096, mode, seed=row, skip=sk), want)
                _stats("row %d %s" % (row, mode), q, st, counters)
        assert 0 < want["open_count"][0] < 4096
    finally:
        q.close()


@pytest.mark.parametrize("counters", [True, False])
def test_deep_frames_interleaved_with_shallow_frames(counters):
    _need_gpu()
    dpts, dnrm, depth, open_count = HS.deep_frames()
    assert depth == HS.DEEP_DEPTH <= HS.ANYHIT_LDS      # the finding: the hemisphere rays stay inside the LDS entries
    spts, snrm, _ = HS.frames("deep", "random")
    n = dpts.shape[0]
    pts = np.ascontiguousarray(np.stack([dpts, spts[:n]], 1).reshape(-1, 3))
    nrm = np.ascontiguousarray(np.stack([dnrm, snrm[:n]], 1).reshape(-1, 3))
    dev = M.ctx("deep")["dev"]
    q = R.RayQuery(dev, counters=counters)
    try:
        got = q.hemisphere(dpts, dnrm, HS.DEEP_SAMPLES, seed=3)
        assert np.array_equal(got["open_count"], open_count)            # the yardstick's
        want, st = dev.hemisphere(pts, nrm, HS.DEEP_SAMPLES, seed=3, stats=True)
        for _ in range(2):                                              # the same call twice
            _same("deep", q.hemisphere(pts, nrm, HS.DEEP_SAMPLES, seed=3), want)
            _stats("deep", q, st, counters)
            _same("deep torch", q.hemisphere(_cuda(pts), _cuda(nrm), HS.DEEP_SAMPLES, seed=3), want)
    finally:
        q.close()


def test_alternating_streams():
    """hemisphere, occluded_filtered and closest alternate on two torch streams on one object: they share the slots, the
    filter rows, the count words (the closest hit's records), the queue words and the overflow buffer."""
    _need_gpu()
    torch.cuda.set_device(0)
    scene = "cornell_plus"
    dev = M.ctx(scene)["dev"]
    pts, nrm, fm, masks, want, _ = _twin(scene, "random", "all", 65, "cosine")
    rays = np.ascontiguousarray(M.ctx(scene)["sets"]["random"][:2000])
    skip = np.ascontiguousarray(np.resize(fm["skip"], 2000))
    occ = dev.occluded_filtered(rays, skip=skip, masks=masks)
    q0 = R.RayQuery(dev)
    try:
        ct, ci = q0.closest(rays)
    finally:
        q0.close()
    torch.cuda.synchronize()
    pts_t, nrm_t, fm_t, rays_t, skip_t = _cuda(pts), _cuda(nrm), _cuda_members(fm), _cuda(rays), _cuda(skip)
    q = R.RayQuery(dev)
    try:
        q.set_masks(masks)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = []
        for _ in range(3):
            with torch.cuda.stream(s1):
                outs.append(("hemisphere", q.hemisphere(pts_t, nrm_t, 65, "cosine", seed=21, point_offset=7, **fm_t)))
            with torch.cuda.stream(s2):
                outs.append(("closest", q.closest(rays_t)))
            with torch.cuda.stream(s1):
                outs.append(("any", q.occluded_filtered(rays_t, skip=skip_t)))
            with torch.cuda.stream(s2):
                outs.append(("hemisphere", q.hemisphere(pts_t, nrm_t, 65, "cosine", seed=21, point_offset=7, **fm_t)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "hemisphere":
                _same("streams", r, want)
            elif kind == "closest":
                assert np.array_equal(_np(r[0]).view(np.uint32), ct.view(np.uint32)) and np.array_equal(_np(r[1]), ci)
            else:
                assert np.array_equal(_np(r), occ)
    finally:
        q.close()


def test_after_set_masks_and_after_update():
    _need_gpu()
    torch.cuda.set_device(0)
    scene = "teapot"
    path, use_bvh = M.scene_path(scene)
    moved = R.Scene(path, use_bvh=use_bvh, image=M.IMG)
    V = RR.deform(moved.vertices(), "jitter")
    pts, nrm, fm, masks, want, _ = _twin(scene, "random", "mask", 64, "cosine", 33)
    none = moved.hemisphere(pts, nrm, 64, seed=21, point_offset=7, **fm)
    assert not np.array_equal(none["open_count"], want["open_count"])
    q = R.RayQuery(moved)                           # resident: the undeformed geometry
    moved.refit(V)                                  # the host scene moves; q keeps its own copy until update
    try:
        _same("no masks", q.hemisphere(pts, nrm, 64, seed=21, point_offset=7, **fm), none)
        q.set_masks(_cuda(masks.view(np.int32)))
        _same("masks", q.hemisphere(pts, nrm, 64, seed=21, point_offset=7, **fm), want)
        assert q.stats()["live_segments"] == pts.shape[0] * 64
        q.update(_cuda(V))
        assert q.stats()["live_segments"] == 0
        new = moved.hemisphere(pts, nrm, 64, seed=21, point_offset=7, masks=masks, **fm)
        assert not np.array_equal(new["open_count"], want["open_count"])
        _same("after update", q.hemisphere(pts, nrm, 64, seed=21, point_offset=7, **fm), new)
        _same("after update, torch", q.hemisphere(_cuda(pts), _cuda(nrm), 64, seed=21, point_offset=7, **_cuda_members(fm)), new)
        ao = q.ambient_occlusion(pts, nrm, 64, skip=fm["skip"], seed=21)
        assert ao.dtype == np.float32 and ao.shape == (pts.shape[0],)
        assert np.array_equal(ao, moved.hemisphere(pts, nrm, 64, seed=21, skip=fm["skip"], masks=masks)["openness"])
    finally:
        q.close()


def test_constant_free_memory():
    """Once the scratch holds n points the device-pointer call allocates nothing, whatever S: free device memory is the
    same after ten rounds."""
    _need_gpu()
    torch.cuda.set_device(0)
    scene = "cornell_plus"
    pts, nrm, fm, masks, want, st = _twin(scene, "random", "all", 200, "cosine")
    n = pts.shape[0]
    frames_t, fm_t = _cuda(np.ascontiguousarray(np.hstack([pts, nrm]))), _cuda_members(fm)
    q = R.RayQuery(M.ctx(scene)["dev"], counters=True)
    try:
        q.reserve(n)
        q.set_masks(masks)
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        opn = torch.empty(n, dtype=torch.float32, device="cuda")
        ho = R.RtHemisphereOut(cnt.data_ptr(), opn.data_ptr())
        rf = R.RtRayFilter(**{k: v.data_ptr() for k, v in fm_t.items()})
        hp = R.RtHemisphereParams(200, 0, 21, 7)
        L = q.L
        L.rt_query_hemisphere.argtypes = [R.P, R.P, R.P, R.I32, R.P, R.P, R.P]

        def round_():
            assert L.rt_query_hemisphere(q.h, R.P(frames_t.data_ptr()), C.byref(rf), n, C.byref(hp), C.byref(ho), None) == 0
        round_()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(10):
            round_()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
        _same("raw call", dict(open_count=cnt, openness=opn), want)
        _stats("raw call", q, st, True)
    finally:
        q.close()


def test_two_to_the_twenty_rays():
    """n * S = 2^20 = 4096 workgroups of work items, more than the library launches: the grid is `blocks`."""
    _need_gpu()
    scene = "cornell_plus"
    pts, nrm, fm, masks, want, st = _twin(scene, "random", "all", 256, "cosine", 4096)
    assert pts.shape[0] * 256 == 1 << 20
    for counters in (True, False):
        q = R.RayQuery(M.ctx(scene)["dev"], counters=counters)
        try:
            q.set_masks(masks)
            _same("2^20", q.hemisphere(pts, nrm, 256, "cosine", seed=21, point_offset=7, **fm), want)
            _stats("2^20", q, st, counters)
        finally:
            q.close()
