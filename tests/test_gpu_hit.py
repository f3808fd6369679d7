"""Hit records on the GPU: rt_query_closest_hit / rtamd.RayQuery.closest_hit.

Every field of closest_hit equals hit_ref.HitRef -- the definition of include/rt_abi.h restated in numpy, which
tests/test_hit_ref.py ties to the oracle's Möller-Trumbore and to the host twin -- evaluated on the oracle's closest
hits (t, index): bit for bit, or NaN on both sides (hit_ref.same).  (t, index) equal RayQuery.closest on the same
object and rt_query_stats is what it is after closest.  Then the edges of a one-thread-per-ray kernel (batch sizes
around the lane, wave and workgroup), field subsets with guard rows behind every output, dynamic geometry against
Scene.hit_records on the host-refit scene, calls of all three kinds sharing the scratch on alternating streams,
residency, edge rays and refused inputs.  The oracle's and HitRef's answers are computed once per scene and shared.
"""
import atexit
import ctypes as C
import functools
import shutil
import tempfile

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import edge_scenes
import hit_ref as H
import oracle_lib as O
import refit_ref as RR
import rtamd as R
from test_gpu_trace_rays import _ray_sets, _same

pytestmark = pytest.mark.gpu

IMG = (16, 16, 1, 1)
SCENES = ["cornell", "cornell:no_bvh", "cornell_plus", "spheres", "teapot", "deep", "big_leaf"]
COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
N_SCALE, N_KEEP, N_HIT, N_EDGE = 20000, 2037, 2000, 600   # N_KEEP: the largest of BATCHES
BATCHES = (0, 1, 63, 64, 65, 255, 256, 257, 2037)
TORCH_DTYPES = {"t": torch.float32, "index": torch.int32, "uv": torch.float32, "normal": torch.float32,
                "position": torch.float32, "material": torch.int32, "front_face": torch.bool}


@functools.lru_cache(maxsize=None)
def _paths():
    d = tempfile.mkdtemp(prefix="hit_scenes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return dict(edge_scenes.write(d))


def _load(cls, scene):
    name, _, flag = scene.partition(":")
    return cls(_paths().get(name) or "%s/%s.scene" % (R.ASSETS, name), use_bvh=flag != "no_bvh", image=IMG)


@functools.lru_cache(maxsize=None)
def _ctx(scene):
    """Per scene, once: the scenes, the ray sets (the first N_KEEP rays of each of test_gpu_trace_rays' sets, plus
    hit_ref's edge rays), the oracle's closest hits and HitRef's records on them."""
    if R.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    torch.cuda.set_device(0)
    orc, dev = _load(O.OracleScene, scene), _load(R.Scene, scene)
    sets = {k: np.ascontiguousarray(v[:N_KEEP], np.float32) for k, v in _ray_sets(orc, np.random.default_rng(1234), N_SCALE).items()}
    sets.update(H.edge_rays(orc.arrays(), np.random.default_rng(99), N_EDGE))
    ref = H.HitRef(orc)
    hit, want = {}, {}
    for k, rays in sets.items():
        hit[k] = orc.closest_hit(rays)[:2]
        want[k] = ref.records(rays, hit[k][0], hit[k][1])
    return dict(orc=orc, dev=dev, sets=sets, hit=hit, want=want, S=orc.info.sphere_count)


def _np(rec):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rec.items()}


def _assert_fields(what, got, want, fields=R.HIT_FIELDS):
    got = _np(got)
    for k in fields:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = H.differing_rows(got[k], want[k])
        assert bad.size == 0, "%s %s: %d rows differ, first %d: gpu %r want %r (index %d, t %r)" % (
            what, k, bad.size, bad[0], got[k][bad[0]], want[k][bad[0]], want["index"][bad[0]], want["t"][bad[0]])


def _head(want, n):
    return {k: v[:n] for k, v in want.items()}


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", SCENES)
def test_fields_bitexact(scene, counters):
    c = _ctx(scene)
    q = R.RayQuery(c["dev"], counters=counters)
    try:
        for name, rays in c["sets"].items():
            rays = np.ascontiguousarray(rays[:N_HIT])
            n = rays.shape[0]
            t_o, i_o, s_o = c["orc"].closest_hit(rays)          # with the counters of exactly these rays
            want = _head(c["want"][name], n)
            rays_t = torch.from_numpy(rays).cuda()
            t_c, i_c = q.closest(rays_t)
            st_c = q.stats()
            got = q.closest_hit(rays_t)
            st_h = q.stats()
            assert list(got) == list(R.HIT_FIELDS)
            for k, v in got.items():
                assert v.device == rays_t.device and v.dtype == TORCH_DTYPES[k] and v.is_contiguous(), (k, v.dtype)
            _assert_fields("%s/%s" % (scene, name), got, want)
            assert _same(t_c.cpu().numpy(), i_c.cpu().numpy(), got["t"].cpu().numpy(), got["index"].cpu().numpy()).size == 0
            assert st_h == st_c, (scene, name, st_c, st_h)
            assert st_h["live_segments"] == n and st_h["hits"] == int((i_o >= 0).sum()) and st_h["misses"] == int((i_o < 0).sum())
            assert st_h["hits_sphere"] == int(((i_o >= 0) & (i_o < c["S"])).sum())
            for k in COUNTERS:
                assert st_h[k] == (s_o[k] if counters else 0), (scene, name, k, s_o[k], st_h[k])
            # the host-pointer path: the same kernel through the object's staging
            _assert_fields("%s/%s host" % (scene, name), q.closest_hit(rays), want)
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres"])
def test_batch_sizes(scene):
    c = _ctx(scene)
    rays_all, want = c["sets"]["random"], c["want"]["random"]
    rays_t = torch.from_numpy(rays_all).cuda()
    q = R.RayQuery(c["dev"])
    try:
        for n in BATCHES:
            for rays in (np.ascontiguousarray(rays_all[:n]), rays_t[:n]):
                got = _np(q.closest_hit(rays))
                for k in R.HIT_FIELDS:
                    assert got[k].shape == (n,) + R.HIT_SHAPES[k][0], (n, k, got[k].shape)
                    assert got[k].dtype == (np.bool_ if k == "front_face" else R.HIT_SHAPES[k][1]), (n, k)
                _assert_fields("%s n=%d" % (scene, n), got, _head(want, n))
                if n:
                    st = q.stats()
                    assert st["live_segments"] == n and st["hits"] == int((want["index"][:n] >= 0).sum())
    finally:
        q.close()


def _pattern(n, k):
    return torch.full((n,) + R.HIT_SHAPES[k][0], 0x5A, dtype=torch.uint8, device="cuda").to(
        torch.uint8 if k == "front_face" else TORCH_DTYPES[k])


@pytest.mark.parametrize("scene", ["cornell_plus", "spheres"])
def test_field_subsets(scene):
    c = _ctx(scene)
    n, guard = 2037, 64
    rays = np.ascontiguousarray(c["sets"]["random"][:n])
    rays_t = torch.from_numpy(rays).cuda()
    want = _head(c["want"]["random"], n)
    q = R.RayQuery(c["dev"])
    f = q.L.rt_query_closest_hit
    try:
        full = _np(q.closest_hit(rays_t))
        _assert_fields(scene, full, want)
        st_full = q.stats()
        subsets = [(k,) for k in R.HIT_FIELDS] + [("uv", "material"), R.HIT_FIELDS, ()]
        for fields in subsets:
            for r in (rays_t, rays):
                got = q.closest_hit(r, fields=fields)
                assert list(got) == [k for k in R.HIT_FIELDS if k in fields]
                _assert_fields("%s %s" % (scene, fields), got, full, fields)
                assert q.stats() == st_full, fields                 # also with no field at all: traversed and counted
            # the raw call on pattern-filled tensors with guard rows behind every output
            buf = {k: _pattern(n + guard, k) for k in R.HIT_FIELDS}
            fill = {k: v.clone() for k, v in buf.items()}
            ho = R.RtHitOut(**{k: buf[k].data_ptr() for k in fields})
            assert f(q.h, R.P(rays_t.data_ptr()), n, C.byref(ho), None) == 0
            torch.cuda.synchronize()
            for k in R.HIT_FIELDS:
                assert torch.equal(buf[k][n:], fill[k][n:]), (fields, k)                  # the guard rows
                if k in fields:
                    w = full[k].view(np.uint8) if k == "front_face" else full[k]
                    assert H.differing_rows(buf[k][:n].cpu().numpy(), w).size == 0, (fields, k)
                else:
                    assert torch.equal(buf[k], fill[k]), (fields, k)                      # not requested: not written
    finally:
        q.close()


@functools.lru_cache(maxsize=None)
def _deformed(scene, deformation):
    """The host-refit scene, the rays over the deformed geometry and the twin's records of the one-shot closest hits."""
    base = _load(R.Scene, scene)
    W = RR.deform(base.vertices(), deformation)
    host = _load(R.Scene, scene)
    host.refit(W)
    arr = host.arrays()
    finite = np.isfinite(arr["triangles"][:, 0:9]).all(axis=1)
    shim = RR.Arrays(arr, triangles=arr["triangles"][finite])
    sets = _ray_sets(shim, np.random.default_rng(1234), 500)
    sets.update(H.edge_rays(arr, np.random.default_rng(98), 500))
    rays = np.ascontiguousarray(np.concatenate(list(sets.values())), np.float32)
    t, index, _ = R.trace_rays(host, rays)
    return dict(W=W, host=host, rays=rays, want=host.hit_records(rays, t, index))


@pytest.mark.parametrize("deformation", ["jitter", "collapse"])
@pytest.mark.parametrize("scene", ["cornell", "deep"])
def test_after_update(scene, deformation):
    c = _ctx(scene)
    d = _deformed(scene, deformation)
    q = R.RayQuery(c["dev"])
    try:
        q.update(d["W"])
        _assert_fields("%s/%s" % (scene, deformation), q.closest_hit(d["rays"]), d["want"])
        _assert_fields("%s/%s tensor" % (scene, deformation), q.closest_hit(torch.from_numpy(d["rays"]).cuda()), d["want"])
        if deformation == "collapse":
            tri = d["want"]["index"] >= c["S"]
            assert np.isnan(d["want"]["normal"][tri]).all()
    finally:
        q.close()


def test_update_and_closest_hit_on_side_streams():
    c = _ctx("cornell")
    A, B = _deformed("cornell", "jitter"), _deformed("cornell", "collapse")
    rays_a, rays_b = torch.from_numpy(A["rays"]).cuda(), torch.from_numpy(B["rays"]).cuda()
    WA, WB = torch.from_numpy(A["W"]).cuda(), torch.from_numpy(B["W"]).cuda()
    q = R.RayQuery(c["dev"])
    try:
        q.reserve(max(rays_a.shape[0], rays_b.shape[0]))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            q.update(WA)
        with torch.cuda.stream(s2):
            got_a = q.closest_hit(rays_a)
        with torch.cuda.stream(s1):
            q.update(WB)
        with torch.cuda.stream(s2):
            got_b = q.closest_hit(rays_b)
        torch.cuda.synchronize()
        _assert_fields("jitter", got_a, A["want"])
        _assert_fields("collapse", got_b, B["want"])
    finally:
        q.close()


def test_shared_scratch_on_alternating_streams():
    c = _ctx("teapot")
    rays = c["sets"]["random"]
    rays_t = torch.from_numpy(rays).cuda()
    tm_t = torch.from_numpy(np.ascontiguousarray(np.float32(1.01) * c["hit"]["random"][0])).cuda()
    q = R.RayQuery(c["dev"])
    try:
        alone = {"hit": _np(q.closest_hit(rays_t)), "occluded": q.occluded(rays_t, tm_t).cpu().numpy(),
                 "closest": [x.cpu().numpy() for x in q.closest(rays_t)]}
        _assert_fields("alone", alone["hit"], c["want"]["random"])
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for k in range(3):
            with torch.cuda.stream(s1):
                outs.append(("hit", q.closest_hit(rays_t)))
            with torch.cuda.stream(s2):
                outs.append(("occluded", q.occluded(rays_t, tm_t)))
            with torch.cuda.stream(s1):
                outs.append(("closest", q.closest(rays_t)))
            with torch.cuda.stream(s2):
                outs.append(("hit", q.closest_hit(rays_t, fields=("normal", "front_face", "index", "t"))))
        s1.synchronize()
        s2.synchronize()
        for k, (kind, r) in enumerate(outs):
            if kind == "hit":
                _assert_fields("call %d" % k, r, alone["hit"], tuple(r))
            elif kind == "occluded":
                assert np.array_equal(r.cpu().numpy(), alone["occluded"]), k
            else:
                assert _same(alone["closest"][0], alone["closest"][1], r[0].cpu().numpy(), r[1].cpu().numpy()).size == 0, k
    finally:
        q.close()


def test_calls_allocate_nothing_once_reserved():
    c = _ctx("teapot")
    rays_t = torch.from_numpy(c["sets"]["random"]).cuda()
    want = c["want"]["random"]
    q = R.RayQuery(c["dev"])
    try:
        q.reserve(rays_t.shape[0])
        got = q.closest_hit(rays_t)                             # also warms torch's allocator for the outputs
        _assert_fields("warm", got, want)
        del got
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        for k in range(10):
            got = q.closest_hit(rays_t)
            if k in (0, 9):
                _assert_fields("round %d" % k, got, want)
            del got
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free0
    finally:
        q.close()


def test_a_batch_larger_than_the_scratch_regrows():
    c = _ctx("teapot")
    names = list(c["sets"])
    rays = np.ascontiguousarray(np.concatenate([c["sets"][k] for k in names]))
    want = {f: np.concatenate([c["want"][k][f] for k in names]) for f in R.HIT_FIELDS}
    q = R.RayQuery(c["dev"])
    try:
        q.reserve(300)
        small = np.ascontiguousarray(rays[:257])
        _assert_fields("small", q.closest_hit(torch.from_numpy(small).cuda()), _head(want, 257))
        _assert_fields("regrown", q.closest_hit(torch.from_numpy(rays).cuda()), want)       # ~60 times the scratch
        _assert_fields("regrown host", q.closest_hit(rays), want)
        _assert_fields("small again", q.closest_hit(small), _head(want, 257))
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["cornell", "spheres"])
def test_edge_rays(scene):
    c = _ctx(scene)
    q = R.RayQuery(c["dev"])
    try:
        for name in ("on_surface", "on_surface_normal", "nan_component", "zero_direction", "non_finite"):
            rays, want = c["sets"][name], c["want"][name]
            for r in (rays, torch.from_numpy(rays).cuda()):
                _assert_fields("%s/%s" % (scene, name), q.closest_hit(r), want)
            miss = want["index"] < 0
            got = q.closest_hit(rays)
            for k in ("uv", "normal", "position"):
                assert not got[k][miss].view(np.uint32).any(), (name, k)        # +0 bit patterns
            assert (got["material"][miss] == -1).all() and not got["front_face"][miss].any()
        assert (c["want"]["on_surface"]["index"] >= 0).any()
        assert np.isnan(c["want"]["nan_component"]["position"]).any() or scene == "spheres"
    finally:
        q.close()


def test_refused_inputs_do_no_work():
    c = _ctx("cornell")
    rays = c["sets"]["random"]
    rays_t = torch.from_numpy(rays).cuda()
    q = R.RayQuery(c["dev"])
    f = q.L.rt_query_closest_hit
    try:
        for x in (rays_t.double(), rays_t[:, :5], rays_t.t().contiguous().t(), rays_t.cpu(), rays_t.reshape(-1),
                  rays.astype(np.float64), rays[:, :5], rays[::2]):
            with pytest.raises(ValueError):
                q.closest_hit(x)
        with pytest.raises(ValueError, match="unknown hit-record field"):
            q.closest_hit(rays_t, fields=("t", "normals"))
        q.closest_hit(rays_t[:100])
        before = q.stats()
        assert before["live_segments"] == 100
        guard = _pattern(rays.shape[0], "normal")
        fill = guard.clone()
        ho = R.RtHitOut(normal=guard.data_ptr())
        for args in ((None, R.P(rays_t.data_ptr()), 8, C.byref(ho), None), (q.h, None, 8, C.byref(ho), None),
                     (q.h, R.P(rays_t.data_ptr()), 8, None, None), (q.h, R.P(rays_t.data_ptr()), -1, C.byref(ho), None)):
            assert f(*args) == -1                               # RT_E_INVALID
            assert b"rt_query_closest_hit" in q.L.rt_last_error()
        assert f(q.h, None, 0, None, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(guard, fill) and q.stats() == before  # nothing ran: the last call is still the 100-ray one
    finally:
        q.close()
