"""Resident ray queries (rt_query_*, rtamd.RayQuery) on the GPU.

closest: bit-exact t (NaN = NaN) and index against the oracle's restatement of the sphere loop +
bvh_closest_hit_distance (scene.cu:338-372, :134-241), with its exact traversal counters -- rt_trace_rays'
contract, now on a resident object.  occluded: the mask bit-exact against tests/anyhit_ref.py (the same
traversal with `closest` held at the ray's bound B), over the ray sets of test_gpu_trace_rays (zero direction
components, origins on vertices, non-finite rays, ...) and bounds at, just below, just above and far from the
closest hit, plus 0, -1, NaN and +inf; at scale against the two relations to the closest hit that are exact
(B = 1e30: occluded <=> index >= 0; B = t_c: never occluded).  The oracle's results are computed once per scene
and shared by the tests.
"""
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads: torch and the library then share one HIP runtime, and a stream of one
               # is a stream of the other (a torch wheel brings its own runtime)

import oracle_lib as O
import rtamd as R
from anyhit_ref import AnyHitRef
from test_gpu_trace_rays import _ray_sets, _same

pytestmark = pytest.mark.gpu

SCENES = [("cornell", True), ("cornell_plus", True), ("spheres", True), ("teapot", True), ("cornell", False)]
COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
N_CLOSEST, N_REF, N_SCALE = 2000, 300, 20000


@functools.lru_cache(maxsize=None)
def _ctx(name, use_bvh):
    """Per scene, computed once: the scenes, the any-hit yardstick, the ray sets (the first N_CLOSEST rays of
    each of the 20,000-ray sets serve the closest test, the first N_REF the yardstick tests) and the oracle's
    closest hits of all of them."""
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    path = "%s/%s.scene" % (R.ASSETS, name)
    img = (16, 16, 1, 1)
    orc, dev = O.OracleScene(path, use_bvh=use_bvh, image=img), R.Scene(path, use_bvh=use_bvh, image=img)
    sets = _ray_sets(orc, np.random.default_rng(1234), N_SCALE)
    hit = {k: orc.closest_hit(v)[:2] for k, v in sets.items()}
    return dict(orc=orc, dev=dev, ref=AnyHitRef(orc), sets=sets, hit=hit)


def _tmax_classes(t_c, rng):
    """One bound per ray, cycling through: 1e30, t_c, the floats just below and just above t_c, 1.01 t_c,
    0.5 t_c, a uniform draw in (0, 2 median t_c), 0, -1, NaN, +inf."""
    n = t_c.shape[0]
    k = np.arange(n) % 11
    fin = t_c[np.isfinite(t_c) & (t_c < np.float32(1e29))]
    med = np.float32(np.median(fin)) if fin.size else np.float32(1.0)
    with np.errstate(all="ignore"):
        cls = [np.full(n, 1e30, np.float32), t_c, np.nextafter(t_c, np.float32(-np.inf)),
               np.nextafter(t_c, np.float32(np.inf)), np.float32(1.01) * t_c, np.float32(0.5) * t_c,
               (rng.random(n) * 2 * med).astype(np.float32), np.zeros(n, np.float32), np.full(n, -1, np.float32),
               np.full(n, np.nan, np.float32), np.full(n, np.inf, np.float32)]
    tm = np.empty(n, np.float32)
    for c, v in enumerate(cls):
        tm[k == c] = np.asarray(v, np.float32)[k == c]
    return tm


@functools.lru_cache(maxsize=None)
def _ref(name, use_bvh):
    """The yardstick's answers, once per scene: per ray set, the first N_REF rays with tmax = None and with
    the per-ray bound classes: {set: (rays, tmax, mask_none, ctr_none, mask_tmax, ctr_tmax)}."""
    c = _ctx(name, use_bvh)
    rng = np.random.default_rng(77)
    out = {}
    for k, rays in c["sets"].items():
        r = np.ascontiguousarray(rays[:N_REF])
        tm = _tmax_classes(c["hit"][k][0][:N_REF], rng)
        m0, c0 = c["ref"].batch(r, None)
        m1, c1 = c["ref"].batch(r, tm)
        out[k] = (r, tm, m0, c0, m1, c1)
    return out


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene,use_bvh", SCENES)
def test_closest_bitexact(scene, use_bvh, counters):
    c = _ctx(scene, use_bvh)
    q = R.RayQuery(c["dev"], counters=counters)
    try:
        for name, rays in c["sets"].items():
            rays = np.ascontiguousarray(rays[:N_CLOSEST])
            t_o, i_o, s_o = c["orc"].closest_hit(rays)
            t_g, i_g = q.closest(rays)
            bad = _same(t_o, i_o, t_g, i_g)
            assert bad.size == 0, "%s/%s: %d rays differ, first %s: oracle (%r, %d) gpu (%r, %d)" % (
                scene, name, bad.size, bad[:1], t_o[bad[0]], i_o[bad[0]], t_g[bad[0]], i_g[bad[0]])
            st = q.stats()
            assert st["live_segments"] == N_CLOSEST
            assert st["hits"] == int((i_o >= 0).sum()) and st["misses"] == int((i_o < 0).sum())
            assert st["hits_sphere"] == int(((i_o >= 0) & (i_o < c["orc"].info.sphere_count)).sum())
            for k in COUNTERS:
                assert st[k] == (s_o[k] if counters else 0), (scene, name, k, s_o[k], st[k])
    finally:
        q.close()


@pytest.mark.parametrize("scene", ["teapot", "spheres"])
def test_batch_sizes(scene):
    c = _ctx(scene, True)
    rays_all = c["sets"]["random"]
    t_all, i_all = c["hit"]["random"]
    q = R.RayQuery(c["dev"])
    try:
        for n in (0, 1, 63, 64, 65, 2037):
            rays = np.ascontiguousarray(rays_all[:n])
            t_g, i_g = q.closest(rays)
            assert t_g.shape == (n,) and i_g.shape == (n,)
            assert _same(t_all[:n], i_all[:n], t_g, i_g).size == 0, n
            m = q.occluded(rays)
            assert m.shape == (n,) and m.dtype == np.bool_
            assert np.array_equal(m, i_all[:n] >= 0), n
            m = q.occluded(rays, np.ascontiguousarray(t_all[:n]))
            assert not m.any(), n
    finally:
        q.close()


@pytest.mark.parametrize("scene,use_bvh", SCENES)
def test_occluded_against_anyhit_ref(scene, use_bvh):
    c = _ctx(scene, use_bvh)
    q = R.RayQuery(c["dev"])
    try:
        for name, (rays, tm, m0, _, m1, _) in _ref(scene, use_bvh).items():
            for what, tmax, want in (("None", None, m0), ("classes", tm, m1)):
                got = q.occluded(rays, tmax)
                assert set(np.unique(got.view(np.uint8))) <= {0, 1}
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, "%s/%s tmax=%s: %d rays differ, first %s (class %s): ref %d gpu %d" % (
                    scene, name, what, bad.size, bad[:1], bad[:1] % 11, want[bad[0]], got[bad[0]])
                st = q.stats()
                assert st["live_segments"] == N_REF and st["hits"] == int(want.sum())
                assert st["misses"] == N_REF - int(want.sum())
    finally:
        q.close()


@pytest.mark.parametrize("scene,use_bvh", SCENES)
def test_occluded_against_closest_at_scale(scene, use_bvh):
    c = _ctx(scene, use_bvh)
    q = R.RayQuery(c["dev"])
    try:
        for name, rays in c["sets"].items():
            t_c, index = c["hit"][name]
            ok = ~np.isnan(t_c)
            m = q.occluded(rays)
            bad = np.nonzero((m != (index >= 0)) & ok)[0]
            assert bad.size == 0, "%s/%s tmax=None: %d rays differ from index >= 0, first %s" % (
                scene, name, bad.size, bad[:1])
            m = q.occluded(rays, t_c)
            bad = np.nonzero(m & ok)[0]
            assert bad.size == 0, "%s/%s tmax=t_c: %d rays occluded, first %s" % (scene, name, bad.size, bad[:1])
    finally:
        q.close()


@pytest.mark.parametrize("scene,use_bvh", SCENES)
def test_occluded_counters_on_unoccluded_rays(scene, use_bvh):
    """On rays the yardstick finds unoccluded the traversal visits a fixed node set whatever the order, so
    Pn/Iv/Tt and the sphere tests equal the yardstick's sums."""
    c = _ctx(scene, use_bvh)
    q = R.RayQuery(c["dev"], counters=True)
    try:
        total = 0
        for name, (rays, tm, m0, c0, m1, c1) in _ref(scene, use_bvh).items():
            for tmax, mask, ctr in ((None, m0, c0), (tm, m1, c1)):
                keep = ~mask
                if not keep.any():
                    continue
                total += int(keep.sum())
                got = q.occluded(np.ascontiguousarray(rays[keep]), None if tmax is None else np.ascontiguousarray(tmax[keep]))
                assert not got.any()
                st = q.stats()
                want = ctr[keep].sum(0)
                assert [st[k] for k in COUNTERS] == [int(v) for v in want], (scene, name, tmax is None)
                assert st["hits"] == 0 and st["misses"] == int(keep.sum())
        assert total > 0
    finally:
        q.close()


def test_residency():
    """One object through growing, shrinking and reserved scratch gives what a fresh object gives."""
    c = _ctx("teapot", True)
    rays = c["sets"]["random"]
    t_c = c["hit"]["random"][0]

    def fresh(kind, n):
        f = R.RayQuery(c["dev"])
        try:
            r = np.ascontiguousarray(rays[:n])
            return f.closest(r) if kind == "closest" else f.occluded(r, np.ascontiguousarray(np.float32(1.01) * t_c[:n]))
        finally:
            f.close()
    q = R.RayQuery(c["dev"])
    try:
        for step in (("closest", 65), ("occluded", 2037), ("closest", 64), ("reserve", 5000), ("occluded", 1)):
            if step[0] == "reserve":
                q.reserve(step[1])
                continue
            kind, n = step
            r = np.ascontiguousarray(rays[:n])
            if kind == "closest":
                got, want = q.closest(r), fresh(kind, n)
                assert _same(want[0], want[1], got[0], got[1]).size == 0, step
                assert _same(t_c[:n], c["hit"]["random"][1][:n], got[0], got[1]).size == 0, step
            else:
                got = q.occluded(r, np.ascontiguousarray(np.float32(1.01) * t_c[:n]))
                assert np.array_equal(got, fresh(kind, n)), step
    finally:
        q.close()


def test_torch_streams():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    torch.cuda.set_device(0)
    c = _ctx("teapot", True)
    n = 5000
    base = np.ascontiguousarray(c["sets"]["random"][:n])
    perm = np.random.default_rng(5).permutation(n)
    rays = np.ascontiguousarray(base[perm])
    tm = np.ascontiguousarray((np.float32(1.01) * c["hit"]["random"][0][:n])[perm])
    q = R.RayQuery(c["dev"])
    try:
        t_n, i_n = q.closest(rays)                                   # the numpy (host) path
        m_n, m0_n = q.occluded(rays, tm), q.occluded(rays)
        base_t, tm_t, perm_t = torch.from_numpy(base).cuda(), torch.from_numpy(tm).cuda(), torch.from_numpy(perm).cuda()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            rays_t = base_t.index_select(0, perm_t)                  # produced on s, consumed in stream order
            t_t, i_t = q.closest(rays_t)
            m_t = q.occluded(rays_t, tm_t)
            m0_t = q.occluded(rays_t)
        s.synchronize()
        assert t_t.device == rays_t.device and i_t.device == rays_t.device and m_t.device == rays_t.device
        assert (t_t.dtype, i_t.dtype, m_t.dtype) == (torch.float32, torch.int32, torch.bool)
        assert t_t.shape == (n,) and i_t.shape == (n,) and m_t.shape == (n,)
        assert _same(t_n, i_n, t_t.cpu().numpy(), i_t.cpu().numpy()).size == 0
        assert np.array_equal(m_n, m_t.cpu().numpy()) and np.array_equal(m0_n, m0_t.cpu().numpy())
        assert set(np.unique(m_t.view(torch.uint8).cpu().numpy())) <= {0, 1}
        # two streams alternating calls on one object
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for k in range(3):
            with torch.cuda.stream(s1):
                outs.append(("closest", q.closest(rays_t)))
            with torch.cuda.stream(s2):
                outs.append(("occluded", q.occluded(rays_t, tm_t)))
            with torch.cuda.stream(s1):
                outs.append(("occluded0", q.occluded(rays_t)))
            with torch.cuda.stream(s2):
                outs.append(("closest", q.closest(rays_t)))
        s1.synchronize()
        s2.synchronize()
        for kind, r in outs:
            if kind == "closest":
                assert _same(t_n, i_n, r[0].cpu().numpy(), r[1].cpu().numpy()).size == 0
            else:
                assert np.array_equal(m_n if kind == "occluded" else m0_n, r.cpu().numpy())
        # the old one-shot query on the same rays
        t_o, i_o, _ = R.trace_rays(c["dev"], rays)
        assert _same(t_o, i_o, t_n, i_n).size == 0
        # wrong inputs are refused, nothing is converted
        for x in (rays_t.double(), rays_t[:, :5], rays_t.t().contiguous().t(), rays_t.cpu()):
            with pytest.raises(ValueError):
                q.closest(x)
    finally:
        q.close()
