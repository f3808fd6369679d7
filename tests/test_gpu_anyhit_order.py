"""anyhit_kernel's visit order on the GPU: rt_query_occluded against AnyHitOrderRef (tests/anyhit_ref.py).

The kernel's order is deterministic per ray (near child first, far child pushed, retire at the first accepted
primitive), so its counters are checked on ALL rays, occluded ones included: the mask bit for bit, and
nodes_popped, internal_visits, triangle_tests and sphere_tests equal to the model's sums to the unit.  A kernel
that visits far-first, keeps walking after an accepted primitive, re-tests a leaf or counts a node twice returns
the right mask and fails here (tests/test_anyhit_order_ref.py shows on the CPU that these rays tell the orders
apart).

* general scenes and ray sets (tests/anyhit_order_cases.py), tmax = None and the bound classes;
* the deep chain: rays that fill the 16 LDS stack entries of a lane and go on into the global overflow buffer --
  all lanes alike (axis_plus), retiring with a full stack (solid_plus), each lane with other nodes and another
  depth, just below, at and above the boundary, stopped after popping back into LDS (tilted_plus), and all three
  mixed in every wave (interleaved);
* a grid as large as the library launches, so the last lanes address the end of the overflow buffer;
* closest and occluded alternating on one object: both lay out the one overflow buffer, differently;
* leaves of more than 63 triangles entered as the selected child, as the popped one and as the root.
The yardstick's answers are computed once per process and shared.
"""
import functools

import numpy as np
import pytest
import torch   # before librtamd.so loads (see test_gpu_query.py)

import anyhit_order_cases as K
import edge_scenes as E
import rtamd as R
from test_gpu_trace_rays import _same

pytestmark = pytest.mark.gpu

COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
BOUNDS = ("none", "classes")


@functools.lru_cache(maxsize=None)
def _dev(scene):
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    path, use_bvh = K.scene_path(scene)
    return R.Scene(path, use_bvh=use_bvh, image=K.IMG)


def _check(q, counters, what, rays, tmax, mask, ctr):
    """One occluded call against the model: mask, hits/misses, and the four counters' sums over all rays."""
    n = rays.shape[0]
    got = q.occluded(rays, tmax)
    assert set(np.unique(got.view(np.uint8))) <= {0, 1}
    bad = np.nonzero(got != mask)[0]
    assert bad.size == 0, "%s: %d of %d rays differ, first %s: model %d gpu %d" % (
        what, bad.size, n, bad[:1], mask[bad[0]], got[bad[0]])
    st = q.stats()
    assert st["live_segments"] == n and st["hits"] == int(mask.sum()) and st["misses"] == n - int(mask.sum()), what
    want = [int(v) for v in ctr.sum(0)] if counters else [0, 0, 0, 0]
    assert [st[k] for k in COUNTERS] == want, "%s: Pn/Iv/Tt/sphere tests: gpu %s model %s" % (
        what, [st[k] for k in COUNTERS], want)


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", K.SCENES)
def test_order_exact_counters_on_all_rays(scene, counters):
    q = R.RayQuery(_dev(scene), counters=counters)
    try:
        occluded = 0
        for name, (rays, tm, res) in K.general(scene).items():
            assert rays.shape[0] == K.N_REF                      # every scene keeps all its rays
            for b in BOUNDS:
                mask, ctr = res[b][:2]
                occluded += int(mask.sum())
                _check(q, counters, "%s/%s tmax=%s" % (scene, name, b), rays, None if b == "none" else tm, mask, ctr)
        assert occluded > 0
    finally:
        q.close()


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("n", [64, 65, 1024, 4096])
@pytest.mark.parametrize("name", ["axis_plus", "solid_plus", "tilted_plus", "interleaved"])
def test_deep_stack(name, n, counters):
    rays, tm, res = K.deep(name, n)
    assert rays.shape[0] == (3 * n if name == "interleaved" else n)
    assert max(int(res[b][2].max()) for b in BOUNDS) >= 17        # past the LDS entries
    q = R.RayQuery(_dev("deep"), counters=counters)
    try:
        for b in BOUNDS:
            mask, ctr = res[b][:2]
            _check(q, counters, "deep/%s n=%d tmax=%s" % (name, n, b), rays, None if b == "none" else tm, mask, ctr)
    finally:
        q.close()


def test_whole_grid():
    """2^20 rays = 4096 workgroups of 256 lanes, more than the library ever launches: `blocks` is CUs x the resident
    workgroups per CU of either traversal kernel, 256 x 8 = 2048 on the MI355X (8 waves per SIMD, 17 KB and 18 KB
    of LDS per workgroup; a kernel trace of such a call shows a grid of 524,288 work-items for both kernels), and
    4096 exceeds CUs x residency for any residency up to 16.  So the grid is `blocks`
    and its last lanes address the end of the overflow buffer.  The rays are a fixed permutation of the 3072
    interleaved deep rays, tiled; the model's work is those 3072 rays."""
    rays, tm, res = K.deep("interleaved", 1024)
    assert rays.shape[0] == 3072
    idx = np.random.default_rng(5).permutation(3072)[np.arange(1 << 20) % 3072]
    big = np.ascontiguousarray(rays[idx])
    for counters in (True, False):
        q = R.RayQuery(_dev("deep"), counters=counters)
        try:
            for b in BOUNDS:
                mask, ctr = res[b][:2]
                _check(q, counters, "deep/whole grid tmax=%s" % b, big,
                       None if b == "none" else np.ascontiguousarray(tm[idx]), mask[idx], ctr[idx])
        finally:
            q.close()


@pytest.mark.parametrize("counters", [True, False])
def test_closest_and_occluded_alternate_on_one_object(counters):
    """trace_kernel lays the overflow buffer out as two words per entry from entry 8, anyhit_kernel as one word from
    entry 16: each call must leave nothing the other one reads."""
    n = 1024
    orc = K.oracle("deep")
    rays, tm, res = K.deep("interleaved", n)
    minus = E.interleaved(E.axis_minus(n), E.solid_minus(n), E.tilted_minus(n))
    m_minus = K.model("deep").batch(minus, None)
    hit = {}
    for which, r in (("plus", rays), ("minus", minus)):
        hit[which] = orc.closest_hit(r)
    assert hit["minus"][2]["max_stack"] > 8                        # past trace_kernel's 8 LDS entries
    q = R.RayQuery(_dev("deep"), counters=counters)
    try:
        for rnd in range(3):
            b = BOUNDS[rnd % 2]
            for which, r in (("plus", rays), ("minus", minus)):
                t_o, i_o, s_o = hit[which]
                t_g, i_g = q.closest(r)
                bad = _same(t_o, i_o, t_g, i_g)
                assert bad.size == 0, "round %d closest %s: %d rays differ, first %s: oracle (%r, %d) gpu (%r, %d)" % (
                    rnd, which, bad.size, bad[:1], t_o[bad[0]], i_o[bad[0]], t_g[bad[0]], i_g[bad[0]])
                st = q.stats()
                assert st["hits"] == int((i_o >= 0).sum())
                for k in COUNTERS:
                    assert st[k] == (s_o[k] if counters else 0), (rnd, which, k, s_o[k], st[k])
                if which == "plus":
                    _check(q, counters, "round %d occluded plus tmax=%s" % (rnd, b), rays,
                           None if b == "none" else tm, res[b][0], res[b][1])
                else:
                    _check(q, counters, "round %d occluded minus" % rnd, minus, None, m_minus[0], m_minus[1])
    finally:
        q.close()


@pytest.mark.parametrize("counters", [True, False])
@pytest.mark.parametrize("scene", K.BIG_LEAF_SCENES)
def test_big_leaves(scene, counters):
    rays, tm, res = K.big_leaf(scene)
    ways = res["none"][2]
    if scene.endswith(":no_bvh"):
        assert ways["root"] > 0
    else:
        assert ways["selected"] > 0 and ways["popped"] > 0
    q = R.RayQuery(_dev(scene), counters=counters)
    try:
        for b in BOUNDS:
            mask, ctr, _ = res[b]
            assert mask.any() and (~mask).any()
            _check(q, counters, "%s big-leaf rays tmax=%s" % (scene, b), rays, None if b == "none" else tm, mask, ctr)
    finally:
        q.close()
