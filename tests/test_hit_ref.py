"""The hit records on the host (rt_scene_hit_records, rtamd.Scene.hit_records), without a GPU.

First the yardstick is tied to the oracle: on every triangle hit of the oracle's closest_hit, hit_ref.HitRef's
recomputed t = dot(e2, q) * f equals the oracle's t bit for bit, so the restatement's f and q, and hence u and v, are
the oracle's Möller-Trumbore's; on finite hits the accept test's predicates hold exactly.  Then the twin: rt_scene_hit_records
equals HitRef on every field -- on the shipped and the edge scenes, after rt_scene_refit with a jitter and a collapse
(zero-area triangles: a == 0, NaN normals), on rays with a NaN component, a zero direction and an origin exactly on a
surface, miss rows included -- and refuses bad arguments.  Floats are compared as hit_ref.same does: equal bits, or NaN
on both sides.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import edge_scenes
import hit_ref as H
import oracle_lib as O
import refit_ref as RR
import rtamd as R
from test_gpu_trace_rays import _ray_sets

IMG = (16, 16, 1, 1)
N_RAYS = 20000
SCENES = ["cornell", "cornell:no_bvh", "cornell_plus", "teapot", "deep", "big_leaf"]
HIT_FUNCTIONS = ("rt_query_closest_hit", "rt_query_closest_hit_host", "rt_scene_hit_records")
OUT_FIELDS = ("uv", "normal", "position", "material", "front_face")


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return dict(edge_scenes.write(str(tmp_path_factory.mktemp("hit_scenes"))))


_cache = {}


def _ctx(paths, scene):
    """Per scene, once: the oracle's and the product's scene, the ray sets (test_gpu_trace_rays' plus hit_ref's edge
    rays) and the oracle's closest hits of all of them."""
    if scene not in _cache:
        name, _, flag = scene.partition(":")
        path = paths.get(name) or "%s/%s.scene" % (R.ASSETS, name)
        orc = O.OracleScene(path, use_bvh=flag != "no_bvh", image=IMG)
        dev = R.Scene(path, use_bvh=flag != "no_bvh", image=IMG)
        sets = _ray_sets(orc, np.random.default_rng(1234), N_RAYS)
        sets.update(H.edge_rays(orc.arrays(), np.random.default_rng(99), 2000))
        sets = {k: np.ascontiguousarray(v, np.float32) for k, v in sets.items()}
        hit = {k: orc.closest_hit(v)[:2] for k, v in sets.items()}
        _cache[scene] = dict(orc=orc, dev=dev, sets=sets, hit=hit)
    return _cache[scene]


def _assert_fields(what, got, want, fields=OUT_FIELDS):
    for k in fields:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = H.differing_rows(got[k], want[k])
        assert bad.size == 0, "%s %s: %d rows differ, first %d: got %r want %r (index %d, t %r)" % (
            what, k, bad.size, bad[0], got[k][bad[0]], want[k][bad[0]], want["index"][bad[0]], want["t"][bad[0]])


def _assert_miss_rows(what, rec, index):
    miss = index < 0
    for k in ("uv", "normal", "position"):
        assert not rec[k][miss].view(np.uint32).any(), (what, k)            # +0 bit patterns
    assert (rec["material"][miss] == -1).all() and not rec["front_face"][miss].any(), what


@pytest.mark.parametrize("scene", SCENES)
def test_hitref_recomputes_the_oracles_t(paths, scene):
    c = _ctx(paths, scene)
    ref = H.HitRef(c["orc"])
    S = c["orc"].info.sphere_count
    mat = c["orc"].arrays()["material_indices"]
    total = 0
    for name, rays in c["sets"].items():
        t, index = c["hit"][name]
        rec = ref.records(rays, t, index)
        tri = index >= S
        total += int(tri.sum())
        bad = np.nonzero(tri & ~H.same(rec["t_re"], t))[0]
        assert bad.size == 0, "%s/%s: %d triangle hits with another t, first %d: oracle %r recomputed %r" % (
            scene, name, bad.size, bad[0], t[bad[0]], rec["t_re"][bad[0]])
        fin = tri & np.isfinite(t)
        u, v = rec["uv"][fin, 0], rec["uv"][fin, 1]
        assert (u >= 0).all() and (u <= 1).all() and (v >= 0).all() and (u + v <= 1).all(), (scene, name)
        assert (u + v).dtype == np.float32
        hit = index >= 0
        assert np.array_equal(rec["material"][hit], mat[index[hit]].astype(np.int32)), (scene, name)
        _assert_miss_rows("%s/%s" % (scene, name), rec, index)
    assert total > 1000, (scene, total)


@pytest.mark.parametrize("scene", SCENES + ["spheres"])
def test_host_twin_equals_hitref(paths, scene):
    c = _ctx(paths, scene)
    ref = H.HitRef(c["orc"])
    for name, rays in c["sets"].items():
        t, index = c["hit"][name]
        want = ref.records(rays, t, index)
        got = c["dev"].hit_records(rays, t, index)
        assert list(got) == list(R.HIT_FIELDS)
        assert got["front_face"].dtype == np.bool_ and got["material"].dtype == np.int32
        _assert_fields("%s/%s" % (scene, name), got, want, R.HIT_FIELDS)
        _assert_miss_rows("%s/%s" % (scene, name), got, index)
    # a subset, in any order, gives the same arrays
    rays = c["sets"]["random"]
    t, index = c["hit"]["random"]
    full = c["dev"].hit_records(rays, t, index)
    part = c["dev"].hit_records(rays, t, index, fields=("material", "uv"))
    assert list(part) == ["uv", "material"]
    _assert_fields(scene, part, full, ("uv", "material"))


@pytest.mark.parametrize("deformation", ["jitter", "collapse"])
@pytest.mark.parametrize("scene", ["cornell", "teapot", "deep", "big_leaf"])
def test_host_twin_after_refit(paths, scene, deformation):
    """The twin reads the scene's current triangles.  Its inputs are any (t, index): the undeformed scene's closest
    hits, and random primitives with random distances, so that every kind of refitted record is evaluated."""
    c = _ctx(paths, scene)
    name, _, flag = scene.partition(":")
    sc = R.Scene(paths.get(name) or "%s/%s.scene" % (R.ASSETS, name), image=IMG)
    sc.refit(RR.deform(sc.vertices(), deformation))
    arr = sc.arrays()
    ref = H.HitRef(RR.Arrays(arr))
    if deformation == "collapse":
        assert np.isnan(arr["triangles"][:, 9:12]).all()
    rng = np.random.default_rng(5)
    count = arr["spheres"].shape[0] + arr["triangles"].shape[0]
    for k in ("random", "vertex_origin", "non_finite", "on_surface"):
        rays = c["sets"][k]
        n = rays.shape[0]
        for what, (t, index) in (("hits", c["hit"][k]),
                                 ("drawn", ((rng.random(n) * 10).astype(np.float32), rng.integers(-1, count, n).astype(np.int32)))):
            want = ref.records(rays, t, index)
            got = sc.hit_records(rays, t, index)
            _assert_fields("%s/%s/%s/%s" % (scene, deformation, k, what), got, want, R.HIT_FIELDS)
            _assert_miss_rows("%s/%s/%s" % (scene, deformation, k), got, index)
            if deformation == "collapse":
                tri = index >= arr["spheres"].shape[0]
                assert tri.any() or what == "hits"
                assert np.isnan(got["normal"][tri]).all() and not got["front_face"][tri].any()


def test_every_requested_row_is_written(paths):
    """The raw call on buffers filled with a pattern: every row of a given field is overwritten (miss rows with +0,
    -1, 0), a field whose pointer is NULL is not touched, and t / index are ignored."""
    c = _ctx(paths, "cornell")
    rays = c["sets"]["outward"][:999]
    t, index = (a[:999].copy() for a in c["hit"]["outward"])
    assert (index < 0).any()
    want = H.HitRef(c["orc"]).records(rays, t, index)
    n = rays.shape[0]
    f = R.lib().rt_scene_hit_records
    f.argtypes = [R.P, R.P, R.P, R.P, R.I32, R.P]
    for given in (OUT_FIELDS, ("normal",), ()):
        buf = {k: np.full((n + 1,) + R.HIT_SHAPES[k][0], 0x5A, np.uint8).astype(R.HIT_SHAPES[k][1]) for k in R.HIT_FIELDS}
        fill = {k: v.copy() for k, v in buf.items()}
        ho = R.RtHitOut(**{k: R._ptr(buf[k]) for k in given})
        ho.t, ho.index = (R._ptr(buf["t"]), R._ptr(buf["index"])) if given else (None, None)
        assert f(c["dev"].ptr, R._ptr(rays), R._ptr(t), R._ptr(index), n, C.byref(ho)) == 0
        for k in R.HIT_FIELDS:
            assert buf[k][n:].tobytes() == fill[k][n:].tobytes(), k               # the guard row
            if k in given:
                w = want[k].view(np.uint8) if k == "front_face" else want[k]
                assert H.differing_rows(buf[k][:n], w).size == 0, k
            else:
                assert buf[k].tobytes() == fill[k].tobytes(), k


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message(paths):
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_scene_hit_records.argtypes = [P, P, P, P, I32, P]
    lib.rt_query_closest_hit.argtypes = [P, P, I32, P, P]
    lib.rt_query_closest_hit_host.argtypes = [P, P, I32, P]
    c = _ctx(paths, "cornell")
    sc = c["dev"]
    rays = c["sets"]["random"][:8]
    t, index = (a[:8].copy() for a in c["hit"]["random"])
    normal = np.full((8, 3), 7, np.float32)
    ho = R.RtHitOut(normal=R._ptr(normal))
    r, tp, ip, hp = R._ptr(rays), R._ptr(t), R._ptr(index), C.byref(ho)
    _invalid(lib, lib.rt_scene_hit_records(None, r, tp, ip, 8, hp), "rt_scene_hit_records", "null scene")
    _invalid(lib, lib.rt_scene_hit_records(sc.ptr, None, tp, ip, 8, hp), "rt_scene_hit_records", "null pointer")
    _invalid(lib, lib.rt_scene_hit_records(sc.ptr, r, None, ip, 8, hp), "rt_scene_hit_records", "null pointer")
    _invalid(lib, lib.rt_scene_hit_records(sc.ptr, r, tp, None, 8, hp), "rt_scene_hit_records", "null pointer")
    _invalid(lib, lib.rt_scene_hit_records(sc.ptr, r, tp, ip, 8, None), "rt_scene_hit_records", "null pointer")
    _invalid(lib, lib.rt_scene_hit_records(sc.ptr, r, tp, ip, -1, hp), "rt_scene_hit_records", "negative")
    count = sc.view.sphere_count + sc.view.triangle_count
    far = index.copy()
    far[5] = count
    _invalid(lib, lib.rt_scene_hit_records(sc.ptr, r, tp, R._ptr(far), 8, hp), "rt_scene_hit_records", "index[5]", str(count))
    assert (normal == 7).all()                                                  # a refused call writes nothing
    assert lib.rt_scene_hit_records(sc.ptr, None, None, None, 0, None) == 0    # n == 0: no pointer touched
    # the query calls check the object, the count and the pointers before any HIP call (see test_query_abi.py: a
    # block of zeros stands in for an object no GPU-less box can create)
    obj = R._ptr(np.zeros(1 << 16, np.uint8))
    for fn, name, tail in ((lib.rt_query_closest_hit, "rt_query_closest_hit", (None,)),
                           (lib.rt_query_closest_hit_host, "rt_query_closest_hit_host", ())):
        _invalid(lib, fn(None, r, 8, hp, *tail), name, "null query")
        _invalid(lib, fn(obj, r, -1, hp, *tail), name, "negative")
        _invalid(lib, fn(obj, None, 8, hp, *tail), name, "null pointer")
        _invalid(lib, fn(obj, r, 8, None, *tail), name, "null pointer")
        assert fn(obj, None, 0, None, *tail) == 0
    # the Python wrappers convert nothing silently and know their fields
    for bad in ((rays.astype(np.float64), t, index), (rays[:, :5], t, index), (rays, t.astype(np.float64), index),
                (rays, t, index.astype(np.int64)), (rays, t[:7], index), (rays, t, index[::2])):
        with pytest.raises(ValueError):
            sc.hit_records(*bad)
    with pytest.raises(ValueError, match="unknown hit-record field 'normals'"):
        sc.hit_records(rays, t, index, fields=("uv", "normals"))


def test_rayquery_closest_hit_validates_before_any_library_call():
    import torch
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None       # a library call would raise AttributeError
    with pytest.raises(ValueError, match="unknown hit-record field"):
        q.closest_hit(np.zeros((4, 6), np.float32), fields=("t", "barycentrics"))
    for x in (np.zeros((4, 6), np.float64), np.zeros((4, 5), np.float32), np.zeros((4, 12), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            q.closest_hit(x)
    cases = {"float32": torch.zeros((4, 6), dtype=torch.float64), "shape": torch.zeros((4, 5), dtype=torch.float32),
             "contiguous": torch.zeros((4, 12), dtype=torch.float32)[:, ::2],
             "cuda:0": torch.zeros((4, 6), dtype=torch.float32)}
    for word, x in cases.items():
        with pytest.raises(ValueError, match=word):
            q.closest_hit(x)


def test_header_and_libraries_have_the_hit_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(HIT_FUNCTIONS) <= names and "rt_hit_out;" in text
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(HIT_FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())
    assert C.sizeof(R.RtHitOut) == 7 * C.sizeof(C.c_void_p) and R.lib().rt_abi_version() == 7
