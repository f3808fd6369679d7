"""The refit on the host (rt_scene_refit, rtamd.Scene.refit / .vertices), without a GPU.

First the yardstick is pinned: refit_ref.ClosestRef, which the GPU tests use over refit arrays no oracle scene
exists for, equals the oracle's orc_closest_hit (t, index and all four traversal counters).  Then the twin:
refitting a generated scene with the file's own vertices reproduces the loader's arrays byte for byte, and
under every deformation rt_scene_refit equals refit_ref.refit_numpy (the definition restated) bit for bit,
with children, material indices and everything else untouched and the reorder-key bounds following the
loader's formula.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import edge_scenes
import oracle_lib as O
import refit_ref as RR
import rtamd as R
from test_gpu_trace_rays import _ray_sets, _same

IMG = (16, 16, 1, 1)
REFIT_FUNCTIONS = ("rt_scene_refit", "rt_query_update_triangles", "rt_query_update_triangles_host",
                   "rt_query_read_geometry")
N_REF = 300


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit_scenes")
    out = dict(edge_scenes.write(str(d)))
    for name in ("cornell", "teapot"):
        out[name] = "%s/%s.scene" % (R.ASSETS, name)
    text, V = RR.random_scene()
    out["random400"] = str(d / "random400.scene")
    with open(out["random400"], "w") as f:
        f.write(text)
    out["random400_vertices"] = V
    return out


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _first_diff(a, b):
    rows = np.nonzero((_u32(a) != _u32(b)).any(axis=1))[0]
    return "first differing row %d: %r != %r" % (rows[0], a[rows[0]], b[rows[0]]) if rows.size else ""


@pytest.mark.parametrize("scene", ["cornell", "teapot", "big_leaf", "deep"])
def test_closest_ref_is_the_oracles_closest_hit(paths, scene):
    orc = O.OracleScene(paths[scene], image=IMG)
    ref = RR.ClosestRef(orc)
    for name, rays in _ray_sets(orc, np.random.default_rng(1234), 20000).items():
        rays = np.ascontiguousarray(rays[:N_REF])
        t_o, i_o, s_o = orc.closest_hit(rays)
        t_r, i_r, ctr = ref.batch(rays)
        bad = _same(t_o, i_o, t_r, i_r)
        assert bad.size == 0, "%s/%s: %d rays differ, first %s: oracle (%r, %d) ref (%r, %d)" % (
            scene, name, bad.size, bad[:1], t_o[bad[0]], i_o[bad[0]], t_r[bad[0]], i_r[bad[0]])
        want = [s_o[k] for k in ("nodes_popped", "internal_visits", "triangle_tests", "sphere_tests")]
        assert [int(x) for x in ctr.sum(0)] == want, (scene, name)


def test_refit_with_the_files_vertices_is_the_loaders_output(paths):
    V = paths["random400_vertices"]
    sc = R.Scene(paths["random400"], image=IMG)
    before = sc.arrays()
    tri = before["triangles"]
    assert tri.shape == (400, 12) and before["bvh"].shape[0] > 50
    # the builder's permutation, recovered by matching p1 (random: every p1 is distinct)
    key = {_u32(V[i, 0:3]).tobytes(): i for i in range(V.shape[0])}
    assert len(key) == V.shape[0]
    perm = np.array([key[_u32(tri[i, 0:3]).tobytes()] for i in range(tri.shape[0])])
    assert sorted(perm) == list(range(400)) and not np.array_equal(perm, np.arange(400))
    sc.refit(np.ascontiguousarray(V[perm]))
    after = sc.arrays()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), (k, _first_diff(before[k], after[k]) if before[k].ndim == 2 else "")


@pytest.mark.parametrize("deformation", RR.DEFORMATIONS)
@pytest.mark.parametrize("scene", ["random400", "cornell", "teapot", "big_leaf", "deep"])
def test_scene_refit_equals_the_definition(paths, scene, deformation):
    sc = R.Scene(paths[scene], image=IMG)
    before = sc.arrays()
    W = RR.deform(sc.vertices(), deformation)
    sc.refit(W)
    after = sc.arrays()
    tri_want, bvh_want = RR.refit_numpy(before["bvh"], W)
    assert np.array_equal(_u32(after["triangles"]), _u32(tri_want)), _first_diff(after["triangles"], tri_want)
    assert np.array_equal(_u32(after["bvh"]), _u32(bvh_want)), _first_diff(after["bvh"], bvh_want)
    assert np.array_equal(_u32(after["bvh"][:, 6:8]), _u32(before["bvh"][:, 6:8]))
    for k in ("material_indices", "materials", "spheres", "env"):
        assert before[k].tobytes() == after[k].tobytes(), k
    lo, inv = RR.key_bounds(bvh_want, before["spheres"])
    cam = after["camera"]
    assert np.array_equal(_u32(cam[10:13]), _u32(lo)) and np.array_equal(_u32(cam[13:16]), _u32(inv))
    assert np.array_equal(_u32(np.delete(cam, np.s_[10:16])), _u32(np.delete(before["camera"], np.s_[10:16])))


def test_vertices_reconstructs_the_records(paths):
    sc = R.Scene(paths["cornell"], image=IMG)
    t, V = sc.arrays()["triangles"], sc.vertices()
    assert V.dtype == np.float32 and V.shape == (t.shape[0], 9) and V.flags["C_CONTIGUOUS"]
    assert np.array_equal(V[:, 0:3], t[:, 0:3]) and np.array_equal(V[:, 3:6], t[:, 0:3] + t[:, 3:6])
    assert np.array_equal(V[:, 6:9], t[:, 0:3] + t[:, 6:9])


def test_a_scene_without_triangles_is_a_no_op():
    sc = R.Scene("%s/spheres.scene" % R.ASSETS, image=IMG)
    assert sc.view.triangle_count == 0
    before = sc.arrays()
    f = R.lib().rt_scene_refit
    f.argtypes = [R.P, R.P, R.I32]
    assert f(sc.h, None, 0) == 0
    sc.refit(np.zeros((0, 9), np.float32))
    after = sc.arrays()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message(paths):
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_scene_refit.argtypes = [P, P, I32]
    lib.rt_query_update_triangles.argtypes = [P, P, I32, P]
    lib.rt_query_update_triangles_host.argtypes = [P, P, I32]
    lib.rt_query_read_geometry.argtypes = [P, P, P]
    sc = R.Scene(paths["cornell"], image=IMG)
    V = sc.vertices()
    before = sc.arrays()
    _invalid(lib, lib.rt_scene_refit(None, R._ptr(V), V.shape[0]), "rt_scene_refit", "null")
    _invalid(lib, lib.rt_scene_refit(sc.h, None, V.shape[0]), "rt_scene_refit", "null")
    _invalid(lib, lib.rt_scene_refit(sc.h, R._ptr(V), V.shape[0] - 1), "rt_scene_refit", "triangle_count", str(V.shape[0]))
    _invalid(lib, lib.rt_scene_refit(sc.h, R._ptr(V), 0), "rt_scene_refit", "triangle_count")
    _invalid(lib, lib.rt_query_update_triangles(None, R._ptr(V), V.shape[0], None), "rt_query_update_triangles", "null")
    _invalid(lib, lib.rt_query_update_triangles_host(None, R._ptr(V), V.shape[0]), "rt_query_update_triangles_host", "null")
    _invalid(lib, lib.rt_query_read_geometry(None, None, None), "rt_query_read_geometry", "null")
    after = sc.arrays()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)       # a refused call changes nothing
    # the Python wrapper converts nothing silently
    for x in (V.astype(np.float64), V[:, :8], np.ascontiguousarray(V.reshape(-1)), V[::2], V.tolist(),
              np.zeros((V.shape[0], 18), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            sc.refit(x)
    with pytest.raises(R.RtError, match="triangle_count"):
        sc.refit(np.ascontiguousarray(V[:-1]))


def test_rayquery_update_validates_before_any_library_call():
    import torch
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None       # a library call would raise AttributeError
    for x in (np.zeros((4, 9), np.float64), np.zeros((4, 8), np.float32), np.zeros(36, np.float32),
              np.zeros((4, 18), np.float32)[:, ::2], [[0.0] * 9]):
        with pytest.raises(ValueError):
            q.update(x)
    cases = {"float32": torch.zeros((4, 9), dtype=torch.float64), "shape": torch.zeros((4, 6), dtype=torch.float32),
             "contiguous": torch.zeros((4, 18), dtype=torch.float32)[:, ::2],
             "cuda:0": torch.zeros((4, 9), dtype=torch.float32)}
    for word, x in cases.items():
        with pytest.raises(ValueError, match=word):
            q.update(x)


def test_header_and_libraries_have_the_refit_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(REFIT_FUNCTIONS) <= names
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    for path in (R.LIB_PATH, R.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert set(REFIT_FUNCTIONS) <= set(line.split()[-1] for line in out.splitlines())


def test_abi_version_and_struct_sizes_unchanged():
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtOpts) == 56
    assert C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8
    assert C.sizeof(R.RtScene) == 216 and C.sizeof(R.RtLoadOpts) == 48
