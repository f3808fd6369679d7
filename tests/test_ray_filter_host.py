"""The filtered ray queries on the CPU (rt_abi.h): the host twins rt_scene_closest_filtered and
rt_scene_occluded_filtered against the numpy yardstick (tests/ray_filter_ref.py) on every row of every filter class
(tests/ray_filter_scenes.py), the relations R1-R3, the compatibility with the unfiltered any-hit, the arguments and the
ABI.  No GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import multihit_scenes as M
import oracle_lib as O
import ray_filter_ref as RF
import ray_filter_scenes as FS
import rtamd as R
from anyhit_ref import AnyHitOrderRef

CTR = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
FUNCTIONS = ("rt_query_set_masks", "rt_query_set_masks_host", "rt_query_closest_filtered", "rt_query_occluded_filtered",
             "rt_query_closest_filtered_host", "rt_query_occluded_filtered_host", "rt_scene_closest_filtered",
             "rt_scene_occluded_filtered")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def twin_rows(dev, rays, f):
    """The twins called once per ray: (t, index, occluded, closest counters (n, 4), any-hit counters (n, 4))."""
    L = R.lib()
    fc, fo = L.rt_scene_closest_filtered, L.rt_scene_occluded_filtered
    fc.argtypes = [R.P, R.P, R.P, R.P, R.I32, R.P, R.P, R.P]
    fo.argtypes = [R.P, R.P, R.P, R.P, R.I32, R.P, R.P]
    n = rays.shape[0]
    t, idx, occ = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    cc, ca = np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)
    masks = R._ptr(f["masks"]) if f["masks"] is not None else None
    base = {k: f[k].ctypes.data for k in FS.MEMBERS if f[k] is not None}
    st = R.RtStats()
    scene = dev.ptr
    for i in range(n):
        rf = R.RtRayFilter(**{k: p + 4 * i for k, p in base.items()})
        r = rays.ctypes.data + 24 * i
        assert fc(scene, masks, r, C.byref(rf), 1, t.ctypes.data + 4 * i, idx.ctypes.data + 4 * i, C.byref(st)) == 0
        cc[i] = [getattr(st, k) for k in CTR]
        assert st.hits == (idx[i] >= 0) and st.live_segments == 1
        assert fo(scene, masks, r, C.byref(rf), 1, occ.ctypes.data + i, C.byref(st)) == 0
        ca[i] = [getattr(st, k) for k in CTR]
    return t, idx, occ.view(np.bool_), cc, ca


@pytest.mark.parametrize("scene", FS.SCENES)
def test_twin_equals_yardstick_on_every_row(scene):
    dev = M.ctx(scene)["dev"]
    for name, runs in FS.ref(scene).items():
        for run, e in runs.items():
            f, where = e["filter"], "%s/%s/%s" % (scene, name, run)
            t, idx, occ, cc, ca = twin_rows(dev, e["rays"], f)
            rt, ri, rc, _ = e["closest"]
            ro, ra, _ = e["anyhit"]
            assert np.array_equal(bits(t), bits(rt)), where
            assert np.array_equal(idx, ri), where
            assert np.array_equal(cc, rc), where
            assert np.array_equal(occ, ro), where
            assert np.array_equal(ca, ra), where
            # one call over the whole batch gives the same rows and the counters' sums
            out, st = dev.closest_filtered(e["rays"], masks=f["masks"], stats=True, **FS.members(f))
            assert np.array_equal(bits(out["t"]), bits(rt)) and np.array_equal(out["index"], ri), where
            assert [st[k] for k in CTR] == list(rc.sum(0)) and st["hits"] == (ri >= 0).sum(), where
            assert st["hits_sphere"] == ((ri >= 0) & (ri < dev.view.sphere_count)).sum(), where
            o2, st2 = dev.occluded_filtered(e["rays"], masks=f["masks"], stats=True, **FS.members(f))
            assert np.array_equal(o2, ro) and [st2[k] for k in CTR] == list(ra.sum(0)), where
            assert st2["hits"] == ro.sum() and st2["misses"] == (~ro).sum(), where


def test_sphere_test_is_ray_sphere_at_the_default_lower_bound():
    """The sphere test with lo = kEps is the reference's bit for bit: the yardstick's numpy restatement against
    orc_ray_sphere on every sphere, ray and bound class; the twin (host/ray_filter_math.h's function) equals the
    yardstick on every row by the test above, `spheres` included."""
    c = M.ctx("spheres")
    L = O.lib()
    sph = np.ascontiguousarray(c["dev"].arrays()["spheres"], np.float32)
    assert sph.shape[0] >= 2
    tb = C.c_float()
    hits = 0
    for name, rays in c["sets"].items():
        tm = c["tm"][name]
        for i in range(FS.N_REF):
            ray = np.ascontiguousarray(rays[i])
            for B in (RF.BIG, RF.upper(tm[i])):
                for k in range(sph.shape[0]):
                    want = bool(L.orc_ray_sphere(sph.ctypes.data + 16 * k, ray.ctypes.data, ray.ctypes.data + 12, float(B),
                                                 C.addressof(tb)))
                    got, t = RF.sphere_test(sph[k], ray, RF.K_EPS, B)
                    assert got == want
                    if want:
                        hits += 1
                        assert bits(t) == bits(np.float32(tb.value))
    assert hits > 1000


def test_the_inputs_reach_the_cases():
    """The yardstick alone: the filter classes drive the walks through the cases the kernels have to get right."""
    seen = set()
    S = {s: M.ctx(s)["dev"].view.sphere_count for s in FS.SCENES}
    for scene in FS.SCENES:
        for name, runs in FS.ref(scene).items():
            t0, i0 = runs["none"]["closest"][:2]
            for run, e in runs.items():
                t, idx, ctr, life = e["closest"]
                f = e["filter"]
                if run == "skip":
                    own = (f["skip"] == i0) & (i0 >= 0)
                    if (own & (idx >= 0) & (idx != i0)).any():
                        seen.add("skip changes the answer")
                    if (own & (idx < 0)).any():
                        seen.add("skip turns a hit into a miss")
                if run == "mask" and ((i0 >= 0) & (idx >= 0) & (idx != i0) & (t > t0)).any():
                    seen.add("a mask reveals the surface behind")
                if run == "tmin":
                    far = (i0 >= 0) & (i0 < S[scene]) & (idx == i0) & (t > t0) & (f["tmin"] > t0)
                    if far.any():
                        rec = M.ctx(scene)["dev"].hit_records(e["rays"], t, idx, ("front_face",))["front_face"]
                        if (~rec[far]).any():
                            seen.add("tmin between a sphere's roots returns the far root")
                if (life[:, 2] > 0).any():
                    seen.add("a discarded pop")
                if (life[:, 0] > RF.CLOSEST_LDS).any() and (life[:, 1] > 0).any():
                    seen.add("closest stack past the LDS entries on " + scene)
                if (e["anyhit"][2][:, 0] > RF.ANYHIT_LDS).any() and (e["anyhit"][2][:, 1] > 0).any():
                    seen.add("any-hit stack past the LDS entries on " + scene)
                if run in ("tmax", "all"):
                    neg = RF.upper(0) >= np.array([RF.upper(v) for v in f["tmax"]])
                    if (neg & (ctr[:, 0] == 0)).any() and not (neg & (ctr[:, 0] != 0)).any():
                        seen.add("B <= 0 with Pn = 0")
                if scene == "big_leaf" and (ctr[:, 2] >= 80).any():
                    seen.add("the 80-triangle leaf")
    # an exact-t tie on twins decided by the visit order; the twin's index comes back once the first one is skipped
    m = FS.model("twins", False)
    rays = M.ctx("twins")["sets"]["through"][:64]
    for r in rays:
        t1, i1 = m.closest(r)[:2]
        t2, i2 = m.closest(r, skip=i1)[:2]
        if i1 >= 0 and i2 >= 0 and i2 != i1 and bits(t1) == bits(t2):
            assert np.array_equal(m.tris[i1 - m.S], m.tris[i2 - m.S])      # the twin: the same triangle again
            seen.add("an exact-t tie decided by visit order")
            break
    want = {"skip changes the answer", "skip turns a hit into a miss", "a mask reveals the surface behind",
            "tmin between a sphere's roots returns the far root", "a discarded pop",
            "closest stack past the LDS entries on deep", "closest stack past the LDS entries on teapot",
            "any-hit stack past the LDS entries on deep", "B <= 0 with Pn = 0", "the 80-triangle leaf",
            "an exact-t tie decided by visit order"}
    assert want <= seen, sorted(want - seen)


def _key(t):
    return int(np.float32(t).view(np.uint32))


RELATION_HEADER = "scene set rows not_brute_force_minimum empty_filter_rows differs_from_rt_query_closest"


def relation_counts(scenes=FS.SCENES, teapot_rays=2):
    """R1 and R2 asserted on every row; R3's counts as text lines, one per scene and ray set: the rows compared with
    their brute-force set over all filter runs, how many of them are not its minimum by (t bits, index) (a miss beside
    a non-empty set included), the rows with an empty filter and how many of those differ from rt_query_closest in t
    or index.  R2 is the answer's own primitive tested alone under B; the whole brute-force set, which R3 needs, costs
    a test of every triangle per ray: all rows, but on teapot (126,050 triangles) the first teapot_rays rays of a set."""
    lines = []
    for scene in scenes:
        c = M.ctx(scene)
        n = FS.n_ref(scene)
        n_brute = min(n, teapot_rays) if scene == "teapot" else n
        for name, runs in FS.ref(scene).items():
            rows = not_min = 0
            for run, e in runs.items():
                f, fm = e["filter"], FS.members(e["filter"])
                t, idx = e["closest"][:2]
                m = FS.model(scene, f["masks"] is not None)
                assert np.array_equal(idx >= 0, e["anyhit"][0]), "R1 %s/%s/%s" % (scene, name, run)
                for i in np.nonzero(idx >= 0)[0]:
                    ok, tm = m.is_member(e["rays"][i], int(idx[i]), **m._row(fm, i))
                    assert ok and _key(tm) == _key(t[i]), "R2 %s/%s/%s row %d" % (scene, name, run, i)
                for i, members in enumerate(m.brute_batch(e["rays"][:n_brute], **{k: (None if v is None else v[:n_brute])
                                                                                  for k, v in fm.items()})):
                    rows += 1
                    keys = [(_key(tt), p) for tt, p in members]
                    if idx[i] < 0:
                        # a miss beside a non-empty brute-force set: a box's float entry >= B pruned a triangle whose
                        # float t < B (rt_abi.h, rt_query_occluded); counted with the rows that are not the minimum
                        not_min += bool(members)
                        continue
                    mine = (_key(t[i]), int(idx[i]))
                    assert mine in keys, "R2 %s/%s/%s row %d" % (scene, name, run, i)
                    # accepted t is NaN or >= kEps: unsigned order is numeric order, every NaN last (multi_hit's key)
                    best = min(keys, key=lambda k: (0x7FC00000 if (k[0] & 0x7FFFFFFF) > 0x7F800000 else k[0], k[1]))
                    not_min += best != mine
            t0, i0 = runs["none"]["closest"][:2]
            differs = int(((bits(t0) != bits(c["t_c"][name][:n])) | (i0 != c["i_c"][name][:n])).sum())
            lines.append("%s %s %d %d %d %d" % (scene, name, rows, not_min, n, differs))
    return lines


@pytest.mark.parametrize("scene", FS.SCENES)
def test_relations_hold_on_every_row(scene):
    lines = relation_counts((scene,))
    print("\n".join([RELATION_HEADER] + lines))            # R3 is recorded, not bounded (pytest -s shows it)
    assert len(lines) == len(FS.ref(scene))


@pytest.mark.parametrize("scene", FS.SCENES)
def test_empty_filter_is_the_unfiltered_any_hit(scene):
    """With an empty filter and no masks occluded_filtered is rt_query_occluded's definition bit for bit, counters of
    the pinned order included (AnyHitOrderRef), and Scene's own answer (multi_hit's count >= 1)."""
    c = M.ctx(scene)
    order = AnyHitOrderRef(c["orc"])
    n = FS.n_ref(scene)
    for name, runs in FS.ref(scene).items():
        for run, tmax in (("none", None), ("tmax", runs["tmax"]["filter"]["tmax"])):
            e = runs[run]
            mask, ctr = order.batch(e["rays"], tmax)[:2]
            assert np.array_equal(e["anyhit"][0], mask) and np.array_equal(e["anyhit"][1], ctr), (scene, name, run)
            _, _, occ, _, ca = twin_rows(c["dev"], e["rays"], e["filter"])
            assert np.array_equal(occ, mask) and np.array_equal(ca, ctr), (scene, name, run)
            assert np.array_equal(c["dev"].multi_hit(e["rays"], 1, tmax)[2] >= 1, mask), (scene, name, run)
            null = c["dev"].occluded_filtered(e["rays"]) if tmax is None else c["dev"].occluded_filtered(e["rays"], tmax=tmax)
            assert np.array_equal(null, mask)
    assert n <= FS.N_REF


def test_results_follow_a_refit():
    path, use_bvh = M.scene_path("cornell_plus")
    dev = R.Scene(path, use_bvh=use_bvh, image=M.IMG)
    v = dev.vertices()
    rng = np.random.default_rng(5)
    dev.refit((v * np.float32(1.05) + rng.normal(size=v.shape).astype(np.float32) * np.float32(0.01)).astype(np.float32))
    e = FS.ref("cornell_plus")["random"]["all"]
    f = e["filter"]
    m = RF.RayFilterRef(dev.arrays(), f["masks"])
    t, idx, ctr, _ = m.closest_batch(e["rays"], **FS.members(f))
    occ, ca, _ = m.anyhit_batch(e["rays"], **FS.members(f))
    gt, gi, go, gc, ga = twin_rows(dev, e["rays"], f)
    assert np.array_equal(bits(gt), bits(t)) and np.array_equal(gi, idx) and np.array_equal(gc, ctr)
    assert np.array_equal(go, occ) and np.array_equal(ga, ca)
    assert not np.array_equal(idx, e["closest"][1])            # the geometry did move


def test_outputs_alone_with_guard_rows():
    dev = M.ctx("cornell_plus")["dev"]
    e = FS.ref("cornell_plus")["random"]["all"]
    f, rays = e["filter"], e["rays"]
    n = rays.shape[0]
    L = R.lib()
    fc = L.rt_scene_closest_filtered
    fc.argtypes = [R.P, R.P, R.P, R.P, R.I32, R.P, R.P, R.P]
    rf = R.RtRayFilter(**{k: R._ptr(f[k]) for k in FS.MEMBERS})
    t = np.full(n + 2, 7.5, np.float32)
    assert fc(dev.ptr, R._ptr(f["masks"]), R._ptr(rays), C.byref(rf), n, t.ctypes.data + 4, None, None) == 0
    assert np.array_equal(bits(t[1:-1]), bits(e["closest"][0])) and t[0] == 7.5 and t[-1] == 7.5
    idx = np.full(n + 2, -77, np.int32)
    assert fc(dev.ptr, R._ptr(f["masks"]), R._ptr(rays), C.byref(rf), n, None, idx.ctypes.data + 4, None) == 0
    assert np.array_equal(idx[1:-1], e["closest"][1]) and idx[0] == -77 and idx[-1] == -77
    # each hit-record field alone is rt_scene_hit_records applied to the twin's (t, index)
    want = dev.hit_records(rays, e["closest"][0], e["closest"][1])
    for k in R.HIT_FIELDS:
        got = dev.closest_filtered(rays, masks=f["masks"], fields=(k,), **FS.members(f))
        assert list(got) == [k]
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert dev.closest_filtered(rays, fields=()) == {}
    # a NULL filter struct behaves as a struct of NULLs
    t0, t1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    empty = R.RtRayFilter()
    assert fc(dev.ptr, None, R._ptr(rays), None, n, R._ptr(t0), None, None) == 0
    assert fc(dev.ptr, None, R._ptr(rays), C.byref(empty), n, R._ptr(t1), None, None) == 0
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(t0), bits(FS.ref("cornell_plus")["random"]["none"]["closest"][0]))


def test_masks_from_materials():
    dev = M.ctx("cornell_plus")["dev"]
    mi = dev.arrays()["material_indices"]
    table = np.arange(100, 100 + dev.view.material_count)
    m = R.masks_from_materials(dev, table)
    assert m.dtype == np.uint32 and m.shape == mi.shape and np.array_equal(m, table[mi])
    for bad in (np.zeros(dev.view.material_count, np.float32), np.zeros((2, 2), np.int32), np.array([-1] * 64),
                np.zeros(max(dev.view.material_count - 1, 0), np.uint32)):
        with pytest.raises(ValueError):
            R.masks_from_materials(dev, bad)


# ---------------------------------------------------------------- the boundary
def test_header_declares_and_libraries_export_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(FUNCTIONS) <= names
    assert re.search(r"typedef struct \{[^}]*tmin;[^}]*tmax;[^}]*skip;[^}]*mask;[^}]*\} rt_ray_filter;", text)
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtRayFilter) == 32 and C.sizeof(R.RtHitOut) == 56
    assert C.sizeof(R.RtOpts) == 56 and C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message():
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_query_set_masks.argtypes = [P, P, I32, P]
    lib.rt_query_set_masks_host.argtypes = [P, P, I32]
    lib.rt_query_closest_filtered.argtypes = [P, P, P, I32, P, P]
    lib.rt_query_occluded_filtered.argtypes = [P, P, P, I32, P, P]
    lib.rt_query_closest_filtered_host.argtypes = [P, P, P, I32, P]
    lib.rt_query_occluded_filtered_host.argtypes = [P, P, P, I32, P]
    lib.rt_scene_closest_filtered.argtypes = [P, P, P, P, I32, P, P, P]
    lib.rt_scene_occluded_filtered.argtypes = [P, P, P, P, I32, P, P]
    buf = np.zeros(64, np.float32)
    b = R._ptr(buf)
    ho = R.RtHitOut()
    h = C.byref(ho)
    # null object / scene
    _invalid(lib, lib.rt_query_set_masks(None, b, 1, None), "rt_query_set_masks", "null")
    _invalid(lib, lib.rt_query_set_masks_host(None, b, 1), "rt_query_set_masks_host", "null")
    _invalid(lib, lib.rt_query_closest_filtered(None, b, None, 1, h, None), "rt_query_closest_filtered", "null")
    _invalid(lib, lib.rt_query_occluded_filtered(None, b, None, 1, b, None), "rt_query_occluded_filtered", "null")
    _invalid(lib, lib.rt_query_closest_filtered_host(None, b, None, 1, h), "rt_query_closest_filtered_host", "null")
    _invalid(lib, lib.rt_query_occluded_filtered_host(None, b, None, 1, b), "rt_query_occluded_filtered_host", "null")
    _invalid(lib, lib.rt_scene_closest_filtered(None, None, b, None, 1, b, b, None), "rt_scene_closest_filtered", "null scene")
    _invalid(lib, lib.rt_scene_occluded_filtered(None, None, b, None, 1, b, None), "rt_scene_occluded_filtered", "null scene")
    # The count and the pointers are checked before the object is used (and before any HIP call): a block of zeros
    # stands in for an object no GPU-less box can create (test_query_abi.py); its S + T reads as 0.
    zeros = np.zeros(1 << 16, np.uint8)
    obj = R._ptr(zeros)
    _invalid(lib, lib.rt_query_set_masks(obj, b, 5, None), "count 5")
    _invalid(lib, lib.rt_query_set_masks_host(obj, b, -1), "count -1")
    _invalid(lib, lib.rt_query_set_masks(obj, None, 3, None), "count 3")
    for fn, out in ((lib.rt_query_closest_filtered, h), (lib.rt_query_occluded_filtered, b)):
        _invalid(lib, fn(obj, b, None, -1, out, None), "negative")
        _invalid(lib, fn(obj, None, None, 1, out, None), "null pointer")
        _invalid(lib, fn(obj, b, None, 1, None, None), "null pointer")
        assert fn(obj, None, None, 0, None, None) == 0
    for fn, out in ((lib.rt_query_closest_filtered_host, h), (lib.rt_query_occluded_filtered_host, b)):
        _invalid(lib, fn(obj, b, None, -1, out), "negative")
        _invalid(lib, fn(obj, None, None, 1, out), "null pointer")
        _invalid(lib, fn(obj, b, None, 1, None), "null pointer")
        assert fn(obj, None, None, 0, None) == 0
    scene = M.ctx("cornell")["dev"].ptr
    _invalid(lib, lib.rt_scene_closest_filtered(scene, None, b, None, -1, b, b, None), "negative")
    _invalid(lib, lib.rt_scene_closest_filtered(scene, None, None, None, 1, b, b, None), "null pointer")
    _invalid(lib, lib.rt_scene_occluded_filtered(scene, None, b, None, -1, b, None), "negative")
    _invalid(lib, lib.rt_scene_occluded_filtered(scene, None, None, None, 1, b, None), "null pointer")
    _invalid(lib, lib.rt_scene_occluded_filtered(scene, None, b, None, 1, None, None), "null pointer")
    assert lib.rt_scene_closest_filtered(scene, None, None, None, 0, None, None, None) == 0
    assert lib.rt_scene_occluded_filtered(scene, None, None, None, 0, None, None) == 0


def _unbound_query():
    """A RayQuery with no library and no object behind it (test_query_abi.py): validation that reached the library
    would fail with AttributeError/TypeError instead of ValueError."""
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None
    return q


def test_malformed_members_raise_value_error_before_the_library():
    import torch
    q = _unbound_query()
    dev = M.ctx("cornell")["dev"]
    rays = np.zeros((10, 6), np.float32)
    good = dict(tmin=np.zeros(10, np.float32), tmax=np.zeros(10, np.float32), skip=np.zeros(10, np.int32),
                mask=np.zeros(10, np.uint32))
    for name, a in good.items():
        wrong_type = a.astype(np.float64 if a.dtype == np.float32 else np.int64)
        for bad in (wrong_type, a[:9], np.zeros(20, a.dtype)[::2], a.reshape(10, 1), torch.zeros(10)):
            for call in (q.closest_filtered, q.occluded_filtered, dev.closest_filtered, dev.occluded_filtered):
                with pytest.raises(ValueError, match=name):
                    call(rays, **{name: bad})
    for call in (q.closest_filtered, q.occluded_filtered, dev.closest_filtered, dev.occluded_filtered):
        for bad in (np.zeros((10, 6), np.float64), np.zeros((10, 5), np.float32), np.zeros((10, 12), np.float32)[:, ::2]):
            with pytest.raises(ValueError, match="rays"):
                call(bad)
    for call in (q.closest_filtered, dev.closest_filtered):
        with pytest.raises(ValueError, match="unknown hit-record field"):
            call(rays, fields=("t", "colour"))
    prims = dev.view.sphere_count + dev.view.triangle_count
    for bad in (np.zeros(prims, np.int32), np.zeros(prims + 1, np.uint32), np.zeros((prims, 1), np.uint32),
                np.zeros(2 * prims, np.uint32)[::2]):
        with pytest.raises(ValueError, match="masks"):
            dev.closest_filtered(rays, masks=bad)
        with pytest.raises(ValueError, match="masks"):
            dev.occluded_filtered(rays, masks=bad)
    for bad in (np.zeros(8, np.int32), np.zeros((8, 1), np.uint32), np.zeros(16, np.uint32)[::2], torch.zeros(8),
                torch.zeros(8, dtype=torch.int32)):
        with pytest.raises(ValueError, match="masks"):
            q.set_masks(bad)
    # tensors: check_tensor's rules for the rays and, member by member, for the filter (a CPU tensor: wrong device)
    trays = torch.zeros((10, 6), dtype=torch.float32)
    for call in (q.closest_filtered, q.occluded_filtered):
        with pytest.raises(ValueError, match="cuda:0"):
            call(trays)
    cases = {"tmin": (torch.zeros(10, dtype=torch.float64), "float32"), "tmax": (torch.zeros((10, 1)), "shape"),
             "skip": (torch.zeros(10, dtype=torch.int64), "int32"), "mask": (torch.zeros(10, dtype=torch.float32), "int32"),
             }
    for name, (bad, word) in cases.items():
        with pytest.raises(ValueError, match=word):
            q._filter_tensors(10, **{name: bad})
        with pytest.raises(ValueError, match="torch.Tensor"):
            q._filter_tensors(10, **{name: good[name]})
    with pytest.raises(ValueError, match="contiguous"):
        q._filter_tensors(10, tmin=torch.zeros(20)[::2])
    with pytest.raises(ValueError, match="cuda:0"):
        q._filter_tensors(10, skip=torch.zeros(10, dtype=torch.int32))
