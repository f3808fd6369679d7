"""Box overlap queries on the host (rt_scene_overlap_box, rtamd.Scene.overlap_box), without a GPU.

* The host twin equals the yardstick (tests/overlap_ref.py: box_overlap_math.h's rules in numpy float32) on count, any and
  every entry of every row, padding included, for every scene, box set and K in {1, 2, 8, 64}.
* The any-only walk: the twin's answer, and the yardstick's pinned walk with its counters against the full walk's.
* The inputs do what they are meant to (from the yardstick alone).
* any == (count >= 1) everywhere.
* Meaning: against the float64 restatement, pairs far from the boundary are decided as geometry says.
* The relation to brute force, the refit, optional outputs and guard rows, refused arguments, the ABI, the ValueErrors.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import overlap_ref as OR
import overlap_scenes as S
import refit_ref as RR
import rtamd as R

OVERLAP_FUNCTIONS = ("rt_query_overlap_box", "rt_query_overlap_box_host", "rt_scene_overlap_box")
WITH_TRIANGLES = tuple(s for s in S.SCENES if s != "spheres")
N_PAIRS_TEAPOT = 100     # the brute force evaluates all 126,050 triangles per box
N_MEANING_TEAPOT = 12    # and so does the float64 restatement, at 13 normalised axes each
CAPPED_SETS = ("uniform", "surface")


def _assert_rows(what, got, want, boxes, fields=OR.FIELDS):
    bad = S.differing_rows(got, want, fields)
    assert bad.size == 0, "%s: %d rows differ, first %d (box %r): got %r, want %r" % (
        what, bad.size, bad[0], boxes[bad[0]], {f: got[f][bad[0]] for f in fields}, {f: want[f][bad[0]] for f in fields})


@pytest.mark.parametrize("scene", S.SCENES)
def test_host_twin_equals_yardstick(scene):
    sc = S.scene(scene)
    for name, r in S.ref(scene).items():
        b = r["boxes"]
        for k in S.KS:
            got = sc.overlap_box(b, k, fields=OR.FIELDS)
            assert [got[f].dtype for f in OR.FIELDS] == [np.int32, np.int32, np.uint8]
            assert [got[f].shape for f in OR.FIELDS] == [(len(b), k), (len(b),), (len(b),)]
            _assert_rows("%s/%s k=%d" % (scene, name, k), got, S.rows(scene, name, k), b)


@pytest.mark.parametrize("scene", S.SCENES)
def test_any_only_walk(scene):
    """The pinned any-only walk of the yardstick gives the full walk's any; it never does more work than the full walk and
    exactly the full walk's where nothing is met; a box that is not valid counts nothing.  The twin asked for `any`
    alone (its first-member walk) answers the same.  (The device's counters are held against these in
    test_gpu_overlap.py.)"""
    sc, m = S.scene(scene), S.model(scene)
    stopped = 0
    for name, r in S.ref(scene).items():
        n = min(len(r["boxes"]), 100)
        want = S.rows(scene, name, 1)
        got = sc.overlap_box(r["boxes"], 1, fields=("any",))
        assert list(got) == ["any"] and np.array_equal(got["any"], want["any"]), (scene, name)
        for i in range(n):
            a, ctr = m.any_walk(r["boxes"][i])
            full = tuple(int(x) for x in want["ctr"][i])
            assert a == want["any"][i], (scene, name, i)
            assert all(x <= y for x, y in zip(ctr, full)), (scene, name, i, ctr, full)
            if not a:
                assert ctr == full, (scene, name, i, ctr, full)
            if not OR.valid_box(r["boxes"][i]):
                assert ctr == (0, 0, 0, 0) and full == (0, 0, 0, 0)
            stopped += a and ctr != full
    assert stopped > 0 or scene == "spheres", scene          # stopping early saves work somewhere


def test_inputs_cover_the_paths():
    """Conditions on the inputs, from the yardstick alone.

    The stack: on deep the pinned order holds more than the kernel's 16 LDS entries.  On teapot it cannot: with child1
    entered first and child2 pushed, a node's stack height is the number of its ancestors at which both children met and
    the walk went to child1, and the box that encloses everything (set `all`) meets both children everywhere -- it
    reaches the tree's maximum, which is 15.  The sets reach that maximum; no box can reach more."""
    counts = np.concatenate([S.rows(sc, name, 1)["count"] for sc in S.SCENES for name in S.ref(sc)])
    for k in S.KS:
        assert (counts == 0).sum() >= 10 and (counts == 1).sum() >= 10
        assert k == 1 or ((counts > 0) & (counts < k)).sum() >= 10, k
        assert (counts > k).sum() >= 10, k
    deep = max(int(S.rows("deep", name, 1)["depth"].max()) for name in S.ref("deep"))
    assert deep > OR.ANY_LDS_ENTRIES
    tree_max = int(S.rows("teapot", "all", 1)["depth"].max())
    assert tree_max == 15 and int(S.rows("teapot", "surface", 1)["depth"].max()) == tree_max
    assert max(int(S.rows("big_leaf", name, 1)["max_leaf"].max()) for name in S.ref("big_leaf")) == 80
    ns = S.scene("cornell_plus").view.sphere_count
    idx = np.vstack([S.rows("cornell_plus", name, 64)["index"] for name in S.ref("cornell_plus")])
    both = ((idx >= 0) & (idx < ns)).any(1) & (idx >= ns).any(1)
    assert ns > 0 and both.sum() >= 5                       # boxes meeting a sphere and a triangle
    for scene in ("teapot", "spheres"):
        inside = S.rows(scene, "inside", 1)["count"]
        assert inside.size >= 100 and (inside == 0).all(), scene
    for scene in S.SCENES:                                  # the invalid boxes: three of four, count 0
        b, c = S.ref(scene)["invalid"]["boxes"], S.rows(scene, "invalid", 1)["count"]
        valid = np.array([OR.valid_box(x) for x in b])
        assert (~valid).sum() == 3 * len(b) // 4 and (c[~valid] == 0).all()


@pytest.mark.parametrize("scene", S.SCENES)
def test_any_is_count_at_least_one(scene):
    sc = S.scene(scene)
    for name, b in S.sets(scene).items():
        got = sc.overlap_box(b, 4, fields=OR.FIELDS)
        assert np.array_equal(got["any"], (got["count"] >= 1).astype(np.uint8)), (scene, name)
        assert np.array_equal((got["index"] >= 0).sum(1), np.minimum(got["count"], 4)), (scene, name)
        rows_ok = (np.diff(np.where(got["index"] >= 0, got["index"], 2 ** 31 - 1).astype(np.int64), axis=1) >= 0).all()
        assert rows_ok, (scene, name)                       # ascending, padding last


@pytest.mark.parametrize("scene", WITH_TRIANGLES)
def test_meaning_against_float64(scene):
    """Every (box, triangle) pair of uniform and surface whose float64 gap exceeds 1e-4 D on some axis is a non-member,
    every pair whose float64 overlap is deeper than 1e-4 D on all axes is a member -- of the yardstick's predicate and of
    the twin's rows (a row holds all members where count <= 64).  1e-4 D is about 100 times the float32 projection
    error, a few ulps of D.  Each scene contributes at least 100 decided pairs of each kind."""
    sc, m = S.scene(scene), S.model(scene)
    tol = 1e-4 * S.diagonal(scene)
    ns = m.spheres.shape[0]
    apart = deep = 0
    for name in CAPPED_SETS:
        boxes = S.sets(scene)[name][:N_MEANING_TEAPOT if scene == "teapot" else S.N_REF]
        got = sc.overlap_box(boxes, 64, fields=("index", "count"))
        for i, b in enumerate(boxes):
            gap = OR.triangle_gap64(m.cols, b[0:3], b[3:6])
            mem = OR.triangle_meets(m.cols, b[0:3], b[3:6])
            far, inner = gap > tol, gap < -tol
            assert not mem[far].any(), (scene, name, i, np.nonzero(mem & far)[0][:4])
            assert mem[inner].all(), (scene, name, i, np.nonzero(~mem & inner)[0][:4])
            row = got["index"][i]
            row = row[row >= ns] - ns
            assert not far[row].any(), (scene, name, i)
            if got["count"][i] <= 64:
                assert np.isin(np.nonzero(inner)[0], row).all(), (scene, name, i)
            apart += int(far.sum())
            deep += int(inner.sum())
    print("%s: %d pairs decided apart, %d decided overlapping" % (scene, apart, deep))
    assert apart >= 100 and deep >= 100, (scene, apart, deep)


def relation_counts(scene):
    """{set: (rows with a brute-force member that H lacks, rows looked at)} on the yardstick alone, with the subset and
    failed-ancestor assertions on every row."""
    m = S.model(scene)
    out = {}
    for name, r in S.ref(scene).items():
        n = min(N_PAIRS_TEAPOT if scene == "teapot" else S.N_REF, len(r["boxes"]))
        missing = 0
        for i in range(n):
            b = r["boxes"][i]
            H, B = set(int(x) for x in r["walked"][i]["index"]), set(int(x) for x in m.brute(b))
            assert H <= B, (scene, name, i, sorted(H - B)[:4])
            for prim in B - H:
                assert prim >= m.spheres.shape[0], (scene, name, i, prim)       # every sphere is tested
                assert m.failed_ancestor(b, prim) is not None, (scene, name, i, prim)
            missing += bool(B - H)
        out[name] = (missing, n)
    return out


def write_relation_counts(path):
    """profiles/overlap/relation_counts.txt: python -c "import test_overlap_host as T; T.write_relation_counts(PATH)"
    with tests/ and cuda-raytracer_amd/ on sys.path."""
    with open(path, "w") as f:
        f.write("Rows (boxes) with a brute-force member that H lacks, per scene and box set, from tests/overlap_ref.py alone\n"
                "(test_overlap_host.relation_counts; teapot: the first %d boxes of a set).  uniform and surface are capped\n"
                "at 1 %% of the rows by test_relation_to_brute_force; the other sets, graze included, are not capped.\n\n"
                % N_PAIRS_TEAPOT)
        for scene in S.SCENES:
            for name, (missing, n) in relation_counts(scene).items():
                f.write("%-16s %-8s %4d of %4d\n" % (scene, name, missing, n))


@pytest.mark.parametrize("scene", S.SCENES)
def test_relation_to_brute_force(scene):
    """On the yardstick alone.  H is a subset of the brute-force set; every member of that set which H lacks has an
    ancestor node whose box fails boxes_meet; on uniform and surface, whose coordinates are not taken from a vertex, rows
    with such a member are at most 1 % of the set (profiles/overlap/relation_counts.txt has the counts)."""
    for name, (missing, n) in relation_counts(scene).items():
        print("%s/%s: %d of %d rows lack a brute-force member" % (scene, name, missing, n))
        if name in CAPPED_SETS:
            assert missing <= n // 100, (scene, name, missing)


@pytest.mark.parametrize("scene", ["cornell", "cornell_plus", "deep", "big_leaf", "twins"])
def test_host_twin_after_refit(scene):
    """After Scene.refit the answers follow the new vertices: the twin reads the scene's current triangles and boxes."""
    path, use_bvh = S.CS.MS.scene_path(scene)
    sc = R.Scene(path, use_bvh=use_bvh, image=S.CS.MS.IMG)
    sc.refit(RR.deform(sc.vertices(), "jitter"))
    ref = OR.OverlapRef(sc)
    moved = 0
    for name in ("uniform", "surface", "graze", "thin"):
        b = np.ascontiguousarray(S.ref(scene)[name]["boxes"][:100])
        want = ref.rows(ref.walk(b), 8)
        _assert_rows("%s/%s refit" % (scene, name), sc.overlap_box(b, 8, fields=OR.FIELDS), want, b)
        before = S.rows(scene, name, 8)
        moved += S.differing_rows(want, {f: before[f][:100] for f in OR.FIELDS}).size
    assert moved > 0


def _buffers(n, k):
    return {"index": np.full((n + 2, k), 77, np.int32), "count": np.full(n + 2, 77, np.int32),
            "any": np.full(n + 2, 77, np.uint8)}


GIVEN = (OR.FIELDS, ("index",), ("count",), ("any",), (), ("index", "any"), ("count", "any"))


def check_outputs(call, n, k, want):
    """call(oo) runs the raw function on an RtOverlapOut over arrays with one guard row before and one after the n rows:
    a NULL pointer's array is untouched, nothing is written outside the n rows, the given ones are exact."""
    for given in GIVEN:
        buf = _buffers(n, k)
        fill = {x: v.copy() for x, v in buf.items()}
        oo = R.RtOverlapOut(**{x: R._ptr(buf[x][1:]) for x in given})
        call(oo)
        for x in OR.FIELDS:
            assert buf[x][:1].tobytes() == fill[x][:1].tobytes() and buf[x][n + 1:].tobytes() == fill[x][n + 1:].tobytes(), (given, x)
            if x in given:
                assert S.differing_rows({x: buf[x][1:n + 1]}, want, (x,)).size == 0, (given, x)
            else:
                assert buf[x].tobytes() == fill[x].tobytes(), (given, x)


@pytest.mark.parametrize("k", [1, 8])
def test_optional_outputs_and_guard_rows(k):
    sc = S.scene("cornell_plus")
    b = S.ref("cornell_plus")["uniform"]["boxes"]
    f = R.lib().rt_scene_overlap_box
    f.argtypes = [R.P, R.P, R.I32, R.I32, R.P]

    def call(oo):
        assert f(sc.ptr, R._ptr(b), b.shape[0], k, C.byref(oo)) == 0
    check_outputs(call, b.shape[0], k, S.rows("cornell_plus", "uniform", k))


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message():
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_scene_overlap_box.argtypes = [P, P, I32, I32, P]
    lib.rt_query_overlap_box.argtypes = [P, P, I32, I32, P, P]
    lib.rt_query_overlap_box_host.argtypes = [P, P, I32, I32, P]
    sc = S.scene("cornell")
    b = np.ascontiguousarray(S.sets("cornell")["uniform"][:8])
    d = np.full((8, 4), 7, np.int32)
    oo = R.RtOverlapOut(index=R._ptr(d))
    p, op = R._ptr(b), C.byref(oo)
    # a block of zeros stands in for a query object no GPU-less box can create (see test_query_abi.py): the checks
    # come before the object is used and before any HIP call
    obj = R._ptr(np.zeros(1 << 16, np.uint8))
    calls = ((lambda o, *a: lib.rt_scene_overlap_box(o, *a), "rt_scene_overlap_box", sc.ptr, "null scene"),
             (lambda o, *a: lib.rt_query_overlap_box(o, *a, None), "rt_query_overlap_box", obj, "null query"),
             (lambda o, *a: lib.rt_query_overlap_box_host(o, *a), "rt_query_overlap_box_host", obj, "null query"))
    for fn, name, o, null_word in calls:
        _invalid(lib, fn(None, p, 8, 4, op), name + ":", null_word)
        _invalid(lib, fn(o, p, -1, 4, op), name + ":", "negative")
        for k in (0, -1, 65):
            _invalid(lib, fn(o, p, 8, k, op), name + ":", "outside 1..64")
            _invalid(lib, fn(o, None, 0, k, None), name + ":", "outside 1..64")     # a bad k is refused for n == 0 too
        _invalid(lib, fn(o, None, 8, 4, op), name + ":", "null pointer")
        _invalid(lib, fn(o, p, 8, 4, None), name + ":", "null pointer")
        _invalid(lib, fn(o, p, 2 ** 31 - 1, 2, op), name + ":", "does not fit int32")
        assert fn(o, None, 0, 4, None) == 0                                   # n == 0: no pointer touched
    assert (d == 7).all()                                                     # a refused call writes nothing


def test_python_wrappers_convert_nothing_silently():
    import torch
    sc = S.scene("cornell")
    b = np.ascontiguousarray(S.sets("cornell")["uniform"][:8])
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None       # a library call would raise AttributeError
    for obj in (sc, q):
        for bad in ((b.astype(np.float64), 4), (b[:, :3], 4), (np.zeros((8, 12), np.float32)[:, ::2], 4),
                    (b, 4, ("index", "distance")), (b, 4, "t"), (b, 0), (b, 65), (b, 2.0), (b, True)):
            with pytest.raises(ValueError):
                obj.overlap_box(*bad)
    cases = {"float32": torch.zeros((4, 6), dtype=torch.float64), "shape": torch.zeros((4, 3), dtype=torch.float32),
             "contiguous": torch.zeros((4, 12), dtype=torch.float32)[:, ::2],
             "cuda:0": torch.zeros((4, 6), dtype=torch.float32)}
    for word, x in cases.items():
        with pytest.raises(ValueError, match=word):
            q.overlap_box(x, 4)
    assert sc.overlap_box(b, 4, fields=()) == {}
    assert list(sc.overlap_box(b, 4)) == ["index", "count"]                   # the default fields
    assert list(sc.overlap_box(b, 4, fields=("any", "index"))) == ["index", "any"]
    assert sc.overlap_box(b, np.int64(4), fields="count")["count"].shape == (8,)


def test_header_and_libraries_have_the_overlap_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(OVERLAP_FUNCTIONS) <= names and "rt_overlap_out;" in text
    assert int(re.search(r"#define\s+RT_OVERLAP_K_MAX\s+(\d+)", text).group(1)) == R.OVERLAP_K_MAX == OR.K_MAX == 64
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(OVERLAP_FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtOpts) == 56
    assert C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8
    assert C.sizeof(R.RtOverlapOut) == 3 * C.sizeof(C.c_void_p)
