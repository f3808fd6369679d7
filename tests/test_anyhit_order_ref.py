"""AnyHitOrderRef (tests/anyhit_ref.py), the restated visit order of anyhit_kernel, on the CPU.

* Against AnyHitRef: the order cannot change the answer, nor the work on a ray that is not stopped, so on every
  scene, ray set and bound of tests/anyhit_order_cases.py the masks are identical and Pn, Iv, Tt and the sphere
  tests are identical on every unoccluded ray.
* The constructed deep-chain sets of tests/edge_scenes.py are what they claim: which rays are stopped, how deep
  the model's stack gets, how many pops come from entries >= 16 (the kernel's overflow buffer), and that lanes
  of one wave hold different nodes at the same overflow entry.  Conditions, not tolerances.
* The sets discriminate the order: on each set with occluded rays that test_gpu_anyhit_order.py pins the
  kernel's counters on, the model's summed Pn/Iv/Tt differ from AnyHitRef's.  Were they equal, a kernel that
  visits in AnyHitRef's order (far child first) would pass there.  axis_plus is unoccluded by construction, so
  its counters are order-independent and it is not part of this check; it drives the overflow pops instead.
* The *_minus sets overflow the reference's order: orc.closest_hit reports max_stack > 8, and the sets with
  hits (solid_minus, tilted_minus, the interleaving) hit at least 16 distinct triangles; axis_minus hits none.
"""
import numpy as np
import pytest

import anyhit_order_cases as K
import edge_scenes as E

BOUNDS = ("none", "classes")


@pytest.mark.parametrize("scene", K.SCENES)
def test_order_model_agrees_with_anyhit_ref(scene):
    got, ref = K.general(scene), K.general_ref(scene)
    assert tuple(got) == K.TEAPOT_SETS if scene == "teapot" else len(got) == 8
    unoccluded = 0
    for name, (rays, tm, res) in got.items():
        assert rays.shape == (K.N_REF, 6) and tm.shape == (K.N_REF,)       # no set is cut
        for b in BOUNDS:
            mask, ctr = res[b][:2]
            m0, c0 = ref[name][b]
            bad = np.nonzero(mask != m0)[0]
            assert bad.size == 0, "%s/%s %s: %d masks differ, first %s" % (scene, name, b, bad.size, bad[:1])
            bad = np.nonzero((ctr != c0).any(axis=1) & ~mask)[0]
            assert bad.size == 0, "%s/%s %s: counters differ on %d unoccluded rays, first %s: %s vs %s" % (
                scene, name, b, bad.size, bad[:1], ctr[bad[0]], c0[bad[0]])
            unoccluded += int((~mask).sum())
    assert unoccluded > 0


@pytest.mark.parametrize("scene", K.BIG_LEAF_SCENES)
def test_order_model_agrees_with_anyhit_ref_on_big_leaf_rays(scene):
    rays, tm, res = K.big_leaf(scene)
    p = K.plain(scene)
    for b in BOUNDS:
        mask, ctr, _ = res[b]
        m0, c0 = p.batch(rays, None if b == "none" else tm)
        assert np.array_equal(mask, m0), (scene, b)
        assert np.array_equal(ctr[~mask], c0[~mask]), (scene, b)
        assert mask.any() and (~mask).any()


def test_big_leaf_is_entered_every_way():
    """The leaf of more than 63 triangles is the selected (near or only) child on some rays, the popped far child
    on others, and without a BVH the root."""
    for scene in ("big_leaf", "same65"):
        for b in BOUNDS:
            ways = K.big_leaf(scene)[2][b][2]
            assert ways["selected"] >= 64 and ways["popped"] >= 64 and ways["root"] == 0, (scene, b, ways)
    for b in BOUNDS:
        ways = K.big_leaf("same65:no_bvh")[2][b][2]
        assert ways["root"] >= 64 and ways["selected"] == 0 and ways["popped"] == 0, (b, ways)


def test_axis_plus_walks_the_chain_through_overflow():
    for n in (64, 1024):
        mask, _, depth, opops, _ = K.deep("axis_plus", n)[2]["none"]
        assert not mask.any()
        assert (depth >= 17).all() and (opops >= 1).all()


def test_solid_plus_retires_with_a_full_stack():
    for n in (64, 1024):
        mask, _, depth, opops, _ = K.deep("solid_plus", n)[2]["none"]
        assert mask.all()
        assert (depth >= 17).all() and (opops == 0).all()


def test_tilted_plus_straddles_the_lds_boundary():
    mask, _, depth, opops, opush = K.deep("tilted_plus", 1024)[2]["none"]
    for want in (15, 16, 17, 18):
        assert (depth == want).any(), want
    assert int((mask & (opops >= 1)).sum()) >= 64
    nodes = {}
    for pushes in opush:
        for entry, node in pushes:
            assert entry >= 16
            nodes.setdefault(entry, set()).add(node)
    assert max(len(s) for s in nodes.values()) >= 4, {e: len(s) for e, s in nodes.items()}


@pytest.mark.parametrize("n", [64, 65, 1024, 4096])
def test_interleaved_waves_mix_deep_and_shallow_lanes(n):
    rays, tm, res = K.deep("interleaved", n)
    assert rays.shape == (3 * n, 6) and tm.shape == (3 * n,)
    for b in BOUNDS:
        mask, _, depth, _, _ = res[b]
        for w in range(0, 3 * n - 63, 64):                    # every consecutive 64 rays from a multiple of 64...
            d = depth[w:w + 64]
            assert (d >= 17).any() and (d <= 15).any(), (b, w)
    mask, _, depth, _, _ = res["none"]
    for w in range(0, 3 * min(n, 1024) - 63):                 # ...and from every other start
        d = depth[w:w + 64]
        assert (d >= 17).any() and (d <= 15).any(), w
    assert mask.any() and (~mask).any()


def test_interleaved_is_ray_i_of_each_set_in_turn():
    a, b, c = E.axis_plus(5), E.solid_plus(5), E.tilted_plus(5)
    r = E.interleaved(a, b, c)
    assert r.shape == (15, 6) and r.dtype == np.float32
    assert np.array_equal(r[0::3], a) and np.array_equal(r[1::3], b) and np.array_equal(r[2::3], c)
    for f in (E.axis_plus, E.solid_plus, E.tilted_plus, E.axis_minus, E.solid_minus, E.tilted_minus):
        x = f(7)
        assert x.shape == (7, 6) and x.dtype == np.float32 and np.isfinite(x).all()
        assert np.array_equal(x, f(7))                         # seeded


@pytest.mark.parametrize("name", ["solid_plus", "tilted_plus", "interleaved"])
@pytest.mark.parametrize("n", [64, 65, 1024, 4096])
def test_deep_sets_discriminate_the_order(name, n):
    res, ref = K.deep(name, n)[2], K.deep_ref(name, n)
    for b in BOUNDS:
        mask, ctr = res[b][:2]
        m0, c0 = ref[b]
        assert mask.shape == (3 * n if name == "interleaved" else n,)
        assert np.array_equal(mask, m0)
        assert np.array_equal(ctr[~mask], c0[~mask])
        assert mask.any()
        # Pn and Iv differ on every set; Tt too, except on solid_plus, where the stopping triangle is the first
        # one tested in either order (Tt = 1 per ray)
        for col, what in ((0, "Pn"), (1, "Iv"), (2, "Tt"))[:2 if name == "solid_plus" else 3]:
            assert int(ctr[:, col].sum()) != int(c0[:, col].sum()), (name, n, b, what)


def test_general_and_big_leaf_sets_discriminate_the_order():
    """Beyond the constructed sets: deep's own axis rays from vertices, and the big-leaf rays, also tell the two
    orders apart (summed over the set, each counter)."""
    g, r = K.general("deep")["vertex_origin_axis"][2], K.general_ref("deep")["vertex_origin_axis"]
    for b in BOUNDS:
        assert (g[b][1].sum(0)[:3] != r[b][1].sum(0)[:3]).all(), b
    for scene in ("big_leaf", "same65"):
        rays, tm, res = K.big_leaf(scene)
        for b in BOUNDS:
            _, c0 = K.plain(scene).batch(rays, None if b == "none" else tm)
            assert int(res[b][1][:, 0].sum()) != int(c0[:, 0].sum()), (scene, b)
            assert int(res[b][1][:, 2].sum()) != int(c0[:, 2].sum()), (scene, b)


@pytest.mark.parametrize("name", ["axis_minus", "solid_minus", "tilted_minus", "interleaved"])
def test_minus_sets_overflow_the_reference_order(name):
    n = 1024
    if name == "interleaved":
        rays = E.interleaved(E.axis_minus(n), E.solid_minus(n), E.tilted_minus(n))
    else:
        rays = getattr(E, name)(n)
    t, index, st = K.oracle("deep").closest_hit(rays)
    assert st["max_stack"] > 8
    distinct = len(set(index[index >= 0].tolist()))
    if name == "axis_minus":
        assert distinct == 0
    else:
        assert distinct >= 16, distinct
