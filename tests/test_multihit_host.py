"""Multi-hit queries on the host (rt_scene_multi_hit, rtamd.Scene.multi_hit), without a GPU.

The host twin equals the yardstick (tests/multihit_ref.py: the oracle's own predicates with the bound held and no early
return, sorted by the key) on every field, bit for bit -- count and all K entries of every row, padding included --
over the shipped and the edge scenes, every ray set (non-finite rays included: a NaN t is accepted and sorts last, by
index), tmax = None and the bound classes, K in {1, 2, 8, 64}.  The yardstick alone shows that these inputs truncate
(count > K), leave rows short (count < K) and tie (equal t under two indices among the kept records).  The exact
relations to the other queries, the refused arguments, the refit and the ABI are checked too.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import multihit_ref as M
import multihit_scenes as S
import refit_ref as RR
import rtamd as R
from anyhit_ref import AnyHitRef

MULTI_HIT_FUNCTIONS = ("rt_query_multi_hit", "rt_query_multi_hit_host", "rt_scene_multi_hit")


def _assert_rows(what, got, recs, count, k):
    want = M.rows(recs, k) + (count,)
    assert got[0].shape == want[0].shape and got[0].dtype == np.float32, what
    assert got[1].shape == want[1].shape and got[1].dtype == np.int32, what
    assert got[2].shape == want[2].shape and got[2].dtype == np.int32, what
    bad = M.differing_rows(got, want, k)
    assert bad.size == 0, "%s: %d rows differ, first %d: got t %r index %r count %d, want t %r index %r count %d" % (
        what, bad.size, bad[0], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want[0][bad[0]], want[1][bad[0]],
        want[2][bad[0]])


@pytest.mark.parametrize("scene", S.SCENES)
def test_host_twin_equals_multihitref(scene):
    dev = S.ctx(scene)["dev"]
    short = nan_kept = 0
    for name, (rays, tm, res) in S.ref(scene).items():
        for b in S.BOUNDS:
            recs, count = res[b][:2]
            tmax = None if b == "none" else tm
            for k in S.KS:
                got = dev.multi_hit(rays, k, tmax)
                _assert_rows("%s/%s tmax=%s K=%d" % (scene, name, b, k), got, recs, count, k)
            short += int((count < 64).sum())
            nan_kept += sum(1 for r in recs for h in r if h[0] != h[0])
    assert short > 0                                           # K = 64 leaves rows with count < K
    if scene in ("cornell", "teapot", "big_leaf"):             # a NaN origin: every triangle is accepted with a NaN t
        assert nan_kept > 0, scene


def test_inputs_truncate_and_tie():
    """From the yardstick alone: the inputs reach count > K, and equal t under different indices among kept records."""
    recs, count = S.ref("deep")["solid_plus"][2]["none"][:2]
    assert int(count.max()) == 60
    for k in (1, 2, 8, 32):
        assert (count > k).any()
    assert any((res["none"][1] > 2).any() for _, _, res in S.ref("teapot").values())
    twins = S.ref("twins")["through"][2]["none"]
    assert int(twins[1].max()) >= 2 * 2 * S.TWIN_LAYERS
    for k in (2, 8, 64):
        assert M.kept_ties(twins[0], k) > 0
    # a NaN t sorts after every number, NaNs among themselves by index
    for scene in ("cornell", "teapot"):
        for r in S.ref(scene)["non_finite"][2]["none"][0]:
            keys = [(M.key(h[0]), h[1]) for h in r]
            assert keys == sorted(keys)
            nans = [h[0] != h[0] for h in r]
            assert nans == sorted(nans)


@pytest.mark.parametrize("scene", S.SCENES)
def test_exact_relations(scene):
    """count >= 1 <=> occluded (AnyHitRef) for every bound; for B = 1e30 <=> the oracle's closest index >= 0."""
    c = S.ctx(scene)
    any_ref = AnyHitRef(c["orc"])
    for name, (rays, tm, res) in S.ref(scene).items():
        for b in S.BOUNDS:
            tmax = None if b == "none" else tm
            count = c["dev"].multi_hit(rays, 1, tmax)[2]
            assert np.array_equal(count, res[b][1])
            mask = any_ref.batch(rays, tmax)[0]
            assert np.array_equal(count >= 1, mask), (scene, name, b)
        count = res["none"][1]
        assert np.array_equal(count >= 1, c["i_c"][name] >= 0), (scene, name)


@pytest.mark.parametrize("scene", ["cornell", "cornell_plus", "deep", "big_leaf", "twins"])
def test_host_twin_after_refit(scene):
    """The twin reads the scene's current triangles and boxes.  (The jitter is 1 % of the scene's diagonal per vertex:
    small scenes only, where the yardstick's walk through the inflated boxes stays short.)"""
    path, use_bvh = S.scene_path(scene)
    sc = R.Scene(path, use_bvh=use_bvh, image=S.IMG)
    sc.refit(RR.deform(sc.vertices(), "jitter"))
    ref = M.MultiHitRef(RR.Arrays(sc.arrays()))
    c = S.ctx(scene)
    total = 0
    for name in ("random", "vertex_origin", "non_finite"):
        rays = np.ascontiguousarray(c["sets"][name][:100])
        for tmax in (None, np.ascontiguousarray(c["tm"][name][:100])):
            recs, count = ref.batch(rays, tmax)[:2]
            total += int(count.sum())
            for k in (2, 64):
                _assert_rows("%s/%s refit K=%d" % (scene, name, k), sc.multi_hit(rays, k, tmax), recs, count, k)
    assert total > 0


def test_optional_outputs_and_guard_rows():
    """The raw call on pattern-filled buffers: a NULL pointer's array is untouched, nothing is written past n rows."""
    c = S.ctx("twins")
    rays, tm, res = S.ref("twins")["through"]
    n, k = rays.shape[0], 8
    want = M.rows(res["classes"][0], k) + (res["classes"][1],)
    f = R.lib().rt_scene_multi_hit
    f.argtypes = [R.P, R.P, R.P, R.I32, R.I32, R.P]
    for given in (("t", "index", "count"), ("count",), ("t",), ("index",), ()):
        buf = {"t": np.full((n + 1, k), 7.5, np.float32), "index": np.full((n + 1, k), 77, np.int32),
               "count": np.full(n + 1, 77, np.int32)}
        fill = {x: v.copy() for x, v in buf.items()}
        mo = R.RtMultiHitOut(**{x: R._ptr(buf[x]) for x in given})
        assert f(c["dev"].ptr, R._ptr(rays), R._ptr(tm), n, k, C.byref(mo)) == 0
        for j, x in enumerate(("t", "index", "count")):
            assert buf[x][n:].tobytes() == fill[x][n:].tobytes(), x
            if x in given:
                assert (M.same(buf[x][:n], want[j]) if x == "t" else buf[x][:n] == want[j]).all(), x
            else:
                assert buf[x].tobytes() == fill[x].tobytes(), x


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message():
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_scene_multi_hit.argtypes = [P, P, P, I32, I32, P]
    lib.rt_query_multi_hit.argtypes = [P, P, P, I32, I32, P, P]
    lib.rt_query_multi_hit_host.argtypes = [P, P, P, I32, I32, P]
    sc = S.ctx("cornell")["dev"]
    rays = np.ascontiguousarray(S.ctx("cornell")["sets"]["random"][:8])
    t = np.full((8, 4), 7, np.float32)
    mo = R.RtMultiHitOut(t=R._ptr(t))
    r, mp = R._ptr(rays), C.byref(mo)
    # a block of zeros stands in for a query object no GPU-less box can create (see test_query_abi.py): the checks
    # come before the object is used and before any HIP call
    obj = R._ptr(np.zeros(1 << 16, np.uint8))
    calls = ((lambda o, *a: lib.rt_scene_multi_hit(o, *a), "rt_scene_multi_hit", sc.ptr, "null scene"),
             (lambda o, *a: lib.rt_query_multi_hit(o, *a, None), "rt_query_multi_hit", obj, "null query"),
             (lambda o, *a: lib.rt_query_multi_hit_host(o, *a), "rt_query_multi_hit_host", obj, "null query"))
    for fn, name, o, null_word in calls:
        _invalid(lib, fn(None, r, None, 8, 4, mp), name + ":", null_word)
        _invalid(lib, fn(o, r, None, -1, 4, mp), name + ":", "negative")
        for k in (0, -3, 65):
            _invalid(lib, fn(o, r, None, 8, k, mp), name + ":", "k %d" % k, "1..64")
        _invalid(lib, fn(o, None, None, 8, 4, mp), name + ":", "null pointer")
        _invalid(lib, fn(o, r, None, 8, 4, None), name + ":", "null pointer")
        _invalid(lib, fn(o, r, None, 1 << 30, 64, mp), name + ":", "n * k", str(64 << 30), "int32")
        _invalid(lib, fn(o, None, None, 0, 0, None), name + ":", "k 0")          # k is checked even for n == 0
        assert fn(o, None, None, 0, 4, None) == 0                                 # n == 0: no pointer touched
    assert (t == 7).all()                                                         # a refused call writes nothing
    # the Python wrappers convert nothing silently
    for bad in ((rays.astype(np.float64), 4, None), (rays[:, :5], 4, None), (rays, 0, None), (rays, 65, None),
                (rays, 2.0, None), (rays, 4, np.zeros(7, np.float32)), (rays, 4, np.zeros(8, np.float64))):
        with pytest.raises(ValueError):
            sc.multi_hit(*bad)


def test_rayquery_multi_hit_validates_before_any_library_call():
    import torch
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None       # a library call would raise AttributeError
    good = np.zeros((4, 6), np.float32)
    for bad in ((np.zeros((4, 6), np.float64), 4, None), (np.zeros((4, 5), np.float32), 4, None), (good, 0, None),
                (good, 65, None), (good, 4, np.zeros(3, np.float32))):
        with pytest.raises(ValueError):
            q.multi_hit(*bad)
    cases = {"float32": torch.zeros((4, 6), dtype=torch.float64), "shape": torch.zeros((4, 5), dtype=torch.float32),
             "contiguous": torch.zeros((4, 12), dtype=torch.float32)[:, ::2],
             "cuda:0": torch.zeros((4, 6), dtype=torch.float32)}
    for word, x in cases.items():
        with pytest.raises(ValueError, match=word):
            q.multi_hit(x, 4)


def test_header_and_libraries_have_the_multi_hit_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(MULTI_HIT_FUNCTIONS) <= names and "rt_multi_hit_out;" in text
    assert int(re.search(r"#define\s+RT_MULTI_HIT_MAX\s+(\d+)", text).group(1)) == 64 == R.MULTI_HIT_MAX
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(MULTI_HIT_FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtOpts) == 56
    assert C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8
    assert C.sizeof(R.RtHitOut) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(R.RtMultiHitOut) == 3 * C.sizeof(C.c_void_p)
