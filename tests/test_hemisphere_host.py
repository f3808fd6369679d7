"""Hemisphere visibility queries on the host (rt_scene_hemisphere, rt_hemisphere_rays), no GPU.

* the generator: rt_hemisphere_rays equals the yardstick's rays (tests/hemisphere_ref.py, itself checked against the
  oracle's random_on_sphere on every work item) bit for bit, both modes, S in {1, 3, 64, 65}, with point_offset wrapping
  at 2^32; every finite direction lies in the normal's hemisphere and has unit length; the sample means of
  dot(dir, n) are those of the two distributions;
* R1, exact, on every row: open_count[i] == S - occluded_filtered(the call's own rays, row i's filter).sum();
* the twin equals the yardstick on counts and on all four counters over the first 300 work items per set (16 on
  teapot); openness == float32(count) / float32(S) bit for bit; a split batch with point_offset equals the whole;
  each output alone, with guard rows; the deep frames reach the depth hemisphere_scenes records;
* every refused argument, the ABI and the ValueErrors.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hemisphere_ref as H
import hemisphere_scenes as HS
import multihit_scenes as M
import rtamd as R

FUNCTIONS = ("rt_query_hemisphere", "rt_query_hemisphere_host", "rt_scene_hemisphere", "rt_hemisphere_rays")
COUNTERS = ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Equal bit for bit, a NaN being any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _frames(n=40, seed=5):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)).astype(F)
    nm = rng.normal(size=(n, 3)).astype(F)
    nm[3], nm[4], nm[5], nm[6] = 0, np.nan, (np.inf, 0, 0), (0, 0, 3)
    return p, nm


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("mode", ["cosine", "uniform"])
@pytest.mark.parametrize("samples", [1, 3, 64, 65])
def test_rays_equal_the_yardstick(mode, samples):
    p, nm = _frames()
    for offset in (0, 17, 2 ** 32 - 20, 2 ** 32 - 1):       # the last two wrap inside the batch
        for seed in (0, 0xFFFFFFFF, 12345):
            got = R.hemisphere_rays(p, nm, samples, mode, seed, offset)
            want = H.rays(p, nm, samples, mode, seed, offset)
            assert got.shape == (p.shape[0] * samples, 6) and same(got, want), (mode, samples, offset, seed)
    # the wrap: point_offset + i is taken mod 2^32
    a = R.hemisphere_rays(p, nm, samples, mode, 1, 2 ** 32 - 20)
    b = R.hemisphere_rays(p[20:], nm[20:], samples, mode, 1, 0)
    assert same(a[20 * samples:], b)


@pytest.mark.parametrize("mode", ["cosine", "uniform"])
def test_directions_are_unit_and_in_the_hemisphere(mode):
    p, nm = _frames(200)
    r = R.hemisphere_rays(p, nm, 65, mode, 9, 0)
    nh = np.repeat(H.unit_normals(nm), 65, 0).astype(np.float64)
    d = r[:, 3:6].astype(np.float64)
    ok = np.isfinite(d).all(1) & np.isfinite(nh).all(1)
    assert ok.sum() >= 190 * 65
    dot = (d[ok] * nh[ok]).sum(1)
    ln = np.sqrt((d[ok] * d[ok]).sum(1))
    print("min dot %.3g, max |len - 1| %.3g (4 ulp = %.3g)" % (dot.min(), np.abs(ln - 1).max(), 4 * 2.0 ** -23))
    assert dot.min() >= -1e-6
    assert np.abs(ln - 1).max() <= 4 * 2.0 ** -23
    assert np.array_equal(r[:, :3], np.repeat(p, 65, 0))


def test_sample_means():
    """65,536 samples of one frame (16 rows of it, S = 4096): mean dot(dir, n) is 2/3 in cosine mode and 1/2 in uniform
    mode; the bounds are five standard errors of the exact variances 1/18 and 1/12.  Deterministic: the fixed seed
    passes (measured: see the printed means)."""
    p = np.tile(np.array([[0.5, -1, 2]], F), (16, 1))
    nm = np.tile(np.array([[1, 2, -2]], F), (16, 1))
    nh = np.array([1, 2, -2], np.float64) / 3
    for mode, mean, bound in (("cosine", 2 / 3, 0.005), ("uniform", 1 / 2, 0.006)):
        r = R.hemisphere_rays(p, nm, 4096, mode, 2024, 0)
        assert r.shape[0] == 65536
        m = float((r[:, 3:6].astype(np.float64) @ nh).mean())
        print("%s: mean dot = %.6f (want %.6f +- %.3f)" % (mode, m, mean, bound))
        assert abs(m - mean) <= bound, (mode, m)


# ---------------------------------------------------------------- the twin
def _runs(scene):
    for name in M.ctx(scene)["sets"]:
        pts, nrm, _ = HS.frames(scene, name)
        for run, f in HS.filters(scene, name).items():
            for mode, S in HS.modes_of(run, scene):
                yield name, run, mode, S, pts, nrm, f


@pytest.mark.parametrize("scene", HS.SCENES)
def test_r1_counts_are_the_filtered_anyhit_of_the_calls_own_rays(scene):
    dev = M.ctx(scene)["dev"]
    rows = 16 if scene == "teapot" else None
    for name, run, mode, S, pts, nrm, f in _runs(scene):
        pts, nrm = pts[:rows], nrm[:rows]
        n = pts.shape[0]
        fm = HS.members(f, n)
        out, st = dev.hemisphere(pts, nrm, S, mode, seed=11, masks=f["masks"], stats=True, **fm)
        rays = R.hemisphere_rays(pts, nrm, S, mode, 11)
        per_ray = {k: (None if v is None else np.ascontiguousarray(np.repeat(v, S))) for k, v in fm.items()}
        occ, sta = dev.occluded_filtered(rays, masks=f["masks"], stats=True, **per_ray)
        want = S - occ.reshape(n, S).sum(1)
        what = "%s/%s/%s/%s" % (scene, name, run, mode)
        assert out["open_count"].dtype == np.int32 and np.array_equal(out["open_count"], want), what
        assert np.array_equal(bits(out["openness"]), bits(want.astype(F) / F(S))), what
        assert st["live_segments"] == n * S and st["hits"] == int(occ.sum()) and st["misses"] == n * S - int(occ.sum()), what
        assert [st[k] for k in COUNTERS] == [sta[k] for k in COUNTERS], what


@pytest.mark.parametrize("scene", HS.SCENES)
def test_twin_equals_the_yardstick(scene):
    dev = M.ctx(scene)["dev"]
    for name, runs in HS.ref(scene).items():
        for run, modes in runs.items():
            for mode, (pts, nrm, fm, masks, S, res) in modes.items():
                what = "%s/%s/%s/%s" % (scene, name, run, mode)
                n = pts.shape[0]
                assert n >= 1 and n * S <= HS.n_items(scene) and (res["walked"] == S).all(), what
                out, st = dev.hemisphere(pts, nrm, S, mode, seed=11, masks=masks, stats=True, **fm)
                assert np.array_equal(out["open_count"], res["open_count"]), what
                assert same(R.hemisphere_rays(pts, nrm, S, mode, 11), res["rays"]), what
                assert [st[k] for k in COUNTERS] == [int(v) for v in res["counters"]], what
                assert st["live_segments"] == n * S and st["misses"] == int(res["open_count"].sum()), what


def test_split_batch_with_point_offset_equals_the_whole():
    dev = M.ctx("cornell_plus")["dev"]
    pts, nrm, skip = HS.frames("cornell_plus", "random")
    for mode in ("cosine", "uniform"):
        for base in (0, 2 ** 32 - 100):
            whole = dev.hemisphere(pts, nrm, 65, mode, seed=4, point_offset=base, skip=skip)
            for cut in (1, 100, 299):
                a = dev.hemisphere(pts[:cut], nrm[:cut], 65, mode, seed=4, point_offset=base, skip=np.ascontiguousarray(skip[:cut]))
                b = dev.hemisphere(pts[cut:], nrm[cut:], 65, mode, seed=4, point_offset=(base + cut) % 2 ** 32,
                                   skip=np.ascontiguousarray(skip[cut:]))
                for k in ("open_count", "openness"):
                    assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), (mode, base, cut, k)
    assert not np.array_equal(dev.hemisphere(pts, nrm, 65, seed=5, skip=skip)["open_count"], whole["open_count"])


def test_each_output_alone_with_guard_rows():
    dev = M.ctx("cornell_plus")["dev"]
    pts, nrm, skip = HS.frames("cornell_plus", "random")
    n = pts.shape[0]
    both = dev.hemisphere(pts, nrm, 7, skip=skip)
    assert list(both) == ["open_count", "openness"]
    assert list(dev.hemisphere(pts, nrm, 7, skip=skip, fields=("openness", "open_count"))) == ["open_count", "openness"]
    for k in ("open_count", "openness"):
        assert np.array_equal(dev.hemisphere(pts, nrm, 7, skip=skip, fields=k)[k], both[k])
    f = R.lib().rt_scene_hemisphere
    f.argtypes = [R.P] * 4 + [R.I32] + [R.P] * 3
    fr = np.ascontiguousarray(np.hstack([pts, nrm]))
    rf = R.RtRayFilter(skip=R._ptr(skip))
    hp = R.RtHemisphereParams(7, 0, 0, 0)
    cnt, opn = np.full(n + 2, -77, np.int32), np.full(n + 2, -77, F)
    for ho in (R.RtHemisphereOut(open_count=cnt.ctypes.data + 4), R.RtHemisphereOut(openness=opn.ctypes.data + 4)):
        assert f(dev.ptr, None, R._ptr(fr), C.byref(rf), n, C.byref(hp), C.byref(ho), None) == 0
    assert cnt[0] == cnt[-1] == -77 and opn[0] == opn[-1] == -77
    assert np.array_equal(cnt[1:-1], both["open_count"]) and np.array_equal(bits(opn[1:-1]), bits(both["openness"]))
    rays = np.full((n * 7 + 2, 6), -77, F)
    g = R.lib().rt_hemisphere_rays
    g.argtypes = [R.P, R.I32, R.P, R.P]
    assert g(R._ptr(fr), n, C.byref(hp), rays.ctypes.data + 24) == 0
    assert (rays[0] == -77).all() and (rays[-1] == -77).all() and same(rays[1:-1], R.hemisphere_rays(pts, nrm, 7))


def test_deep_frames_reach_the_recorded_depth():
    """The hemisphere above deep's constructed rays never stacks more than DEEP_DEPTH entries (hemisphere_scenes has the
    argument), so no hemisphere call on it leaves the LDS entries."""
    pts, nrm, depth, open_count = HS.deep_frames()
    assert depth == HS.DEEP_DEPTH and depth <= HS.ANYHIT_LDS
    got = M.ctx("deep")["dev"].hemisphere(pts, nrm, HS.DEEP_SAMPLES, seed=3)["open_count"]
    assert np.array_equal(got, open_count)


def test_ambient_occlusion_of_an_open_and_an_enclosed_point():
    dev = M.ctx("cornell")["dev"]
    a = dev.arrays()
    lo, hi = a["bvh"][0, :3], a["bvh"][0, 3:6]
    inside = ((lo + hi) / 2).astype(F)[None]
    above = np.array([[inside[0, 0], hi[1] + 10, inside[0, 2]]], F)
    up = np.array([[0, 1, 0]], F)
    assert dev.hemisphere(above, up, 256)["open_count"][0] == 256
    assert dev.hemisphere(inside, up, 256, tmax=np.array([1e-3], F))["openness"][0] == 1.0
    assert dev.hemisphere(inside, up, 256, mask=np.zeros(1, np.uint32))["open_count"][0] == 256


# ---------------------------------------------------------------- the boundary
def test_header_declares_and_libraries_export_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(FUNCTIONS) <= names
    assert re.search(r"typedef struct \{\s*int32_t\s+samples;\s*int32_t\s+mode;\s*uint32_t\s+seed;\s*uint32_t\s+point_offset;\s*\} "
                     r"rt_hemisphere_params;", text)
    assert re.search(r"typedef struct \{\s*int32_t \*open_count;\s*float\s+\*openness;\s*\} rt_hemisphere_out;", text)
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    assert int(re.search(r"#define\s+RT_HEMISPHERE_MAX_SAMPLES\s+(\d+)", text).group(1)) == R.HEMISPHERE_MAX_SAMPLES == 4096
    assert re.search(r"#define\s+RT_HEMISPHERE_COSINE\s+0", text) and re.search(r"#define\s+RT_HEMISPHERE_UNIFORM\s+1", text)
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtHemisphereParams) == 16 and C.sizeof(R.RtHemisphereOut) == 16
    assert C.sizeof(R.RtRayFilter) == 32 and C.sizeof(R.RtOpts) == 56 and C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message():
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_query_hemisphere.argtypes = [P, P, P, I32, P, P, P]
    lib.rt_query_hemisphere_host.argtypes = [P, P, P, I32, P, P]
    lib.rt_scene_hemisphere.argtypes = [P, P, P, P, I32, P, P, P]
    lib.rt_hemisphere_rays.argtypes = [P, I32, P, P]
    buf = np.zeros(4096, np.float32)
    b = R._ptr(buf)
    good = C.byref(R.RtHemisphereParams(4, 0, 0, 0))
    out = C.byref(R.RtHemisphereOut(open_count=b))
    none = C.byref(R.RtHemisphereOut())
    # a block of zeros stands in for an object no GPU-less box can create (test_query_abi.py): every check comes before
    # the object is used and before any HIP call
    zeros = np.zeros(1 << 16, np.uint8)
    obj = R._ptr(zeros)
    scene = M.ctx("cornell")["dev"].ptr
    calls = (("rt_query_hemisphere", lambda o, fr, n, hp, ho: lib.rt_query_hemisphere(o, fr, None, n, hp, ho, None), obj),
             ("rt_query_hemisphere_host", lambda o, fr, n, hp, ho: lib.rt_query_hemisphere_host(o, fr, None, n, hp, ho), obj),
             ("rt_scene_hemisphere", lambda o, fr, n, hp, ho: lib.rt_scene_hemisphere(o, None, fr, None, n, hp, ho, None), scene))
    for name, fn, o in calls:
        _invalid(lib, fn(None, b, 1, good, out), name, "null")
        _invalid(lib, fn(o, b, -1, good, out), name, "negative")
        _invalid(lib, fn(o, None, 1, good, out), name, "null frames")
        _invalid(lib, fn(o, b, 1, None, out), name, "null params")
        for s in (0, -1, 4097):
            _invalid(lib, fn(o, b, 1, C.byref(R.RtHemisphereParams(s, 0, 0, 0)), out), name, "samples")
        for m in (-1, 2):
            _invalid(lib, fn(o, b, 1, C.byref(R.RtHemisphereParams(4, m, 0, 0)), out), name, "mode")
        _invalid(lib, fn(o, b, 2 ** 20, C.byref(R.RtHemisphereParams(2048, 0, 0, 0)), out), name, "int32")
        _invalid(lib, fn(o, b, 1, good, None), name, "output")
        _invalid(lib, fn(o, b, 1, good, none), name, "output")
        assert fn(o, None, 0, None, None) == 0              # n == 0 touches no pointer
    _invalid(lib, lib.rt_hemisphere_rays(b, -1, good, b), "rt_hemisphere_rays", "negative")
    _invalid(lib, lib.rt_hemisphere_rays(None, 1, good, b), "rt_hemisphere_rays", "null pointer")
    _invalid(lib, lib.rt_hemisphere_rays(b, 1, good, None), "rt_hemisphere_rays", "null pointer")
    _invalid(lib, lib.rt_hemisphere_rays(b, 1, None, b), "rt_hemisphere_rays", "null params")
    _invalid(lib, lib.rt_hemisphere_rays(b, 1, C.byref(R.RtHemisphereParams(0, 0, 0, 0)), b), "samples")
    _invalid(lib, lib.rt_hemisphere_rays(b, 1, C.byref(R.RtHemisphereParams(4, 7, 0, 0)), b), "mode")
    assert lib.rt_hemisphere_rays(None, 0, None, None) == 0


def _unbound_query():
    """A RayQuery with no library and no object behind it (test_query_abi.py): validation that reached the library
    would fail with AttributeError/TypeError instead of ValueError."""
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None
    return q


def test_malformed_arguments_raise_value_error_before_the_library():
    import torch
    q = _unbound_query()
    dev = M.ctx("cornell")["dev"]
    p, nm = np.zeros((10, 3), F), np.ones((10, 3), F)
    calls = (q.hemisphere, dev.hemisphere)
    for call in calls:
        for bad in (0, -3, 4097, 2.0, True, "4"):
            with pytest.raises(ValueError, match="samples"):
                call(p, nm, bad)
        with pytest.raises(ValueError, match="mode"):
            call(p, nm, 4, mode="stratified")
        for bad in (-1, 2 ** 32, 1.5):
            with pytest.raises(ValueError, match="seed"):
                call(p, nm, 4, seed=bad)
            with pytest.raises(ValueError, match="point_offset"):
                call(p, nm, 4, point_offset=bad)
        for bad in (("count",), (), ("openness", "t")):
            with pytest.raises(ValueError, match="field"):
                call(p, nm, 4, fields=bad)
        for bad in (np.zeros((10, 3), np.float64), np.zeros((10, 4), F), np.zeros((10, 6), F)[:, ::2]):
            with pytest.raises(ValueError, match="points"):
                call(bad, nm, 4)
        for bad in (np.ones((10, 3), np.float64), np.ones((9, 3), F), np.ones(10, F)):
            with pytest.raises(ValueError, match="normals"):
                call(p, bad, 4)
        for name, bad in (("tmin", np.zeros(9, F)), ("tmax", np.zeros(10, np.float64)), ("skip", np.zeros(10, np.int64)),
                          ("mask", np.zeros(10, np.int32))):
            with pytest.raises(ValueError, match=name):
                call(p, nm, 4, **{name: bad})
    with pytest.raises(ValueError, match="int32"):
        R.hemisphere_rays(np.zeros((2 ** 20, 3), F), np.ones((2 ** 20, 3), F), 4096)
    with pytest.raises(ValueError, match="masks"):
        dev.hemisphere(p, nm, 4, masks=np.zeros(3, np.uint32))
    with pytest.raises(ValueError, match="samples"):
        R.hemisphere_rays(p, nm, 0)
    with pytest.raises(ValueError, match="samples"):
        q.ambient_occlusion(p, nm, 0)
    # tensors: check_tensor's rules (a CPU tensor: wrong device), and no mixing of tensors and arrays
    tp, tn = torch.zeros((10, 3)), torch.ones((10, 3))
    with pytest.raises(ValueError, match="cuda:0"):
        q.hemisphere(tp, tn, 4)
    with pytest.raises(ValueError, match="normals"):
        q.hemisphere(tp, nm, 4)
    with pytest.raises(ValueError, match="normals"):
        q.hemisphere(p, tn, 4)
    with pytest.raises(ValueError, match="tmax"):
        q.hemisphere(p, nm, 4, tmax=torch.zeros(10))
