"""Scene.from_mesh on the host (rt_scene_from_mesh): equality with the loader on the description's
canonical scene file, the face index of both entries, every refusal with its message, the Python argument checks and
the host twins downstream.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_build_cases
import bvh_build_ref
import closest_point_scenes
import mesh_cases as MC
import rtamd as R

CASES = ["size_1", "size_5", "size_65", "size_257", "size_4097", "sorted_4097", "line_4097", "same_centroid_4097",
         "chain_5000", "adjacent_floats_6", "denormal_range_6", "points_on_line"]


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mesh_cases"))


_files = {}


def canonical_scene(name, case_dir):
    """Scene(canonical file of case `name`), loaded once and left unchanged."""
    if name not in _files:
        path = MC.write_canonical(MC.case(name), os.path.join(case_dir, name + ".canonical.scene"))
        _files[name] = MC.from_file(path)
    return _files[name]


# ---------------------------------------------------------------- equality with the loader

@pytest.mark.parametrize("as_indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("name", CASES)
def test_from_mesh_equals_canonical_file(case_dir, name, as_indexed):
    want = canonical_scene(name, case_dir)
    got = MC.from_mesh(MC.case(name, as_indexed))
    assert MC.differences(got, want) == []


@pytest.mark.parametrize("name", CASES)
def test_from_mesh_equals_the_build_cases_file(case_dir, name):
    """bvh_build_cases.write's file names its materials differently and carries its own image line."""
    want = R.Scene(bvh_build_cases.write(name, case_dir))
    for as_indexed in (False, True):
        assert MC.differences(MC.from_mesh(MC.case(name, as_indexed)), want) == []


def cornell_description(name="cornell_plus"):
    """A shipped scene's own triangles, spheres and materials read back through arrays() (cornell_plus has spheres)."""
    a = R.Scene(os.path.join(R.ASSETS, name + ".scene")).arrays()
    t = a["triangles"]
    soup = np.ascontiguousarray(np.hstack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]]), np.float32)
    S = a["spheres"].shape[0]
    return dict(vertices=soup, materials=a["materials"], face_materials=a["material_indices"][S:],
                spheres=a["spheres"], sphere_materials=a["material_indices"][:S], camera=MC.CAMERA, sky=MC.SKY)


@pytest.mark.parametrize("name", ["cornell", "cornell_plus"])
def test_from_mesh_cornell(case_dir, name):
    d = cornell_description(name)
    assert d["spheres"].shape[0] == (2 if name == "cornell_plus" else 0) and d["vertices"].shape[0] > 0
    want = MC.from_file(MC.write_canonical(d, os.path.join(case_dir, name + ".canonical.scene")))
    assert MC.differences(MC.from_mesh(d), want) == []
    V, F = MC.indexed(d["vertices"])
    assert MC.differences(MC.from_mesh(dict(d, vertices=V, faces=F)), want) == []


def test_from_mesh_spheres_only(case_dir):
    d = cornell_description()
    d = dict(d, vertices=np.zeros((0, 3), np.float32), face_materials=None)
    want = MC.from_file(MC.write_canonical(d, os.path.join(case_dir, "spheres_only.scene")))
    got = MC.from_mesh(d)
    assert got.view.triangle_count == 0 and got.view.sphere_count == d["spheres"].shape[0]
    assert MC.differences(got, want) == []
    assert got.face_index.shape == (0,)


def test_from_mesh_no_bvh(case_dir):
    d = MC.case("size_257")
    want = MC.from_file(MC.write_canonical(d, os.path.join(case_dir, "no_bvh.scene")), use_bvh=False)
    got = MC.from_mesh(d, use_bvh=False)
    assert got.view.bvh_node_count == 1
    assert MC.differences(got, want) == []


@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("mats", [False, True])
@pytest.mark.parametrize("override", [False, True])
def test_from_mesh_optional_parts(case_dir, camera, sky, mats, override):
    d = MC.case("size_65", True, with_materials=mats, camera=camera, sky=sky)
    kw = dict(image=(24, 10, 3, 2), exposure=0.75) if override else dict(image=None, exposure=None)
    path = MC.write_canonical(d, os.path.join(case_dir, "optional_%d%d%d.scene" % (camera, sky, mats)))
    want, got = MC.from_file(path, **kw), MC.from_mesh(d, **kw)
    assert MC.differences(got, want) == []
    assert (got.view.width, got.view.height) == ((24, 10) if override else (1920, 1080))


def test_from_mesh_camera_is_normalised_like_the_loaders(case_dir):
    d = dict(MC.case("size_5"), camera=((1.0, 2.0, 3.0), (0.3, -0.2, 2.0), (0.1, 3.0, 0.2), 33.3))
    want = MC.from_file(MC.write_canonical(d, os.path.join(case_dir, "camera.scene")))
    assert MC.differences(MC.from_mesh(d), want) == []


# ---------------------------------------------------------------- face index

def records(soup):
    """The loader's ray-tracing records of (n, 9) vertices in numpy float32."""
    v = np.asarray(soup, np.float32).reshape(-1, 3, 3)
    p1, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    a, b = e2, e1
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(np.float32)
    with np.errstate(all="ignore"):
        s = np.float32(1.0) / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        return np.hstack([p1, e1, e2, s[:, None] * n]).astype(np.float32)


@pytest.mark.parametrize("name", CASES)
def test_face_index(case_dir, name):
    soup, mats = bvh_build_cases.vertices(name), bvh_build_cases.materials(name)
    _, perm = bvh_build_ref.build(soup, mats)
    for scene in (MC.from_mesh(MC.case(name)), MC.from_mesh(MC.case(name, True)), canonical_scene(name, case_dir)):
        fi = scene.face_index
        assert fi.dtype == np.int32 and fi.shape == (soup.shape[0],)
        assert np.array_equal(np.sort(fi), np.arange(soup.shape[0]))            # a permutation
        assert np.array_equal(fi, perm)
        a = scene.arrays()
        assert a["triangles"].tobytes() == records(soup[fi]).tobytes()
        assert np.array_equal(a["material_indices"], mats[fi])


def test_face_index_of_a_shipped_scene_file():
    s = R.Scene(os.path.join(R.ASSETS, "teapot.scene"))
    fi = s.face_index
    assert np.array_equal(np.sort(fi), np.arange(s.view.triangle_count))
    assert not np.array_equal(fi, np.arange(s.view.triangle_count))


def test_face_index_does_not_depend_on_the_thread_count(case_dir):
    """One child process with RT_BVH_THREADS=1 (the serial recursion); the default here builds subtrees in parallel."""
    np.save(os.path.join(case_dir, "threads_in.npy"), bvh_build_cases.vertices("size_4097"))
    code = ("import sys, numpy as np\nsys.path[:0] = %r\nimport rtamd as R\n"
            "s = R.Scene.from_mesh(np.load(%r), image=(16, 16, 1, 1))\nnp.save(%r, s.face_index)\n"
            % ([os.path.dirname(R.__file__)], os.path.join(case_dir, "threads_in.npy"),
               os.path.join(case_dir, "threads_out.npy")))
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, RT_BVH_THREADS="1"))
    serial = np.load(os.path.join(case_dir, "threads_out.npy"))
    assert np.array_equal(serial, MC.from_mesh(MC.case("size_4097")).face_index)


# ---------------------------------------------------------------- refusals

TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 2, 2]], np.float32)
FACES = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3]], np.int32)


def refused(m, match, **kw):
    rc, msg = MC.raw_call(m[0], **kw)
    assert rc == -1 and match in msg, (rc, msg)


def test_refuses_null_arguments_and_counts():
    good = MC.raw_desc(TRI, FACES)
    assert MC.raw_call(good[0]) == (0, "")
    refused(good, "null argument", null_mesh=True)
    refused(good, "null argument", null_out=True)
    for k in ("vertex_count", "triangle_count", "sphere_count", "material_count"):
        refused(MC.raw_desc(TRI, FACES, **{k: -1}), "negative count")
    refused(MC.raw_desc(None, FACES, vertex_count=5), "null vertices with 3 triangles")
    refused(MC.raw_desc(TRI[:4], None, triangle_count=1), "a soup of 1 triangles needs 3 vertices, not 4")
    refused(MC.raw_desc(TRI[:3], None, triangle_count=2), "a soup of 2 triangles needs 6 vertices, not 3")
    refused(MC.raw_desc(TRI, FACES, sphere_count=0x7fffffff - 2), "null spheres")
    sph = np.zeros((1, 4), np.float32)
    refused(MC.raw_desc(TRI, FACES, spheres=sph, sphere_count=0x7fffffff - 2), "does not fit int32")


def test_device_entry_refuses_a_host_build_device():
    """rt_scene_from_mesh_device with opts->bvh_device < 0: refused before any pointer is read and before any HIP call."""
    import ctypes as C
    L = R.lib()
    m, keep = MC.raw_desc(TRI, FACES)
    o = R.RtLoadOpts()
    L.rt_default_load_opts(C.byref(o))
    assert o.bvh_device == -1
    h = R.P()
    L.rt_scene_from_mesh_device.argtypes = [R.P, R.P, R.P, R.P]
    assert L.rt_scene_from_mesh_device(C.byref(m), C.byref(o), None, C.byref(h)) == -1
    assert "opts->bvh_device must name the device the arrays are on" in L.rt_last_error().decode()
    assert not h


def test_refuses_material_problems():
    refused(MC.raw_desc(TRI, FACES, face_materials=[0, 0, 0]), "material indices without a material table")
    refused(MC.raw_desc(TRI, FACES, spheres=[[0, 0, 0, 1]], sphere_materials=[0]),
            "material indices without a material table")
    refused(MC.raw_desc(TRI, FACES, materials=MC.MATERIALS, material_count=65536), "more than 65535 materials")
    refused(MC.raw_desc(TRI, FACES, materials=MC.MATERIALS, face_materials=[0, 4, 5]),
            "triangle 2 has a material index outside the table of 5 materials")
    refused(MC.raw_desc(TRI, FACES, materials=MC.MATERIALS, face_materials=[7, 4, 5]),
            "triangle 0 has a material index outside the table of 5 materials")
    refused(MC.raw_desc(TRI, FACES, materials=MC.MATERIALS, spheres=[[0, 0, 0, 1], [1, 1, 1, 1]], sphere_materials=[4, 5]),
            "sphere 1 has a material index outside the table of 5 materials")
    assert MC.raw_call(MC.raw_desc(TRI, FACES, materials=MC.MATERIALS, face_materials=[0, 4, 3])[0]) == (0, "")


def test_refuses_a_bad_image():
    refused(MC.raw_desc(TRI, FACES), "scene image must be at least 2x2", image=(1, 16, 1, 1))
    refused(MC.raw_desc(TRI, FACES), "scene image must be at least 2x2", image=(16, 16, -1, 1))


@pytest.mark.parametrize("value", [-1, 5, -2 ** 31, 2 ** 31 - 1])
@pytest.mark.parametrize("where", ["first", "last"])
def test_refuses_a_bad_vertex_index(value, where):
    n = 300
    faces = np.tile(FACES, (n // 3, 1))
    t = 0 if where == "first" else n - 1
    faces[t, 1] = value
    verts = TRI.copy()
    verts[4] = np.nan                                   # referenced by nobody; and the index check comes first
    refused(MC.raw_desc(verts, faces), "triangle %d has a vertex index outside [0, 5)" % t)
    faces[5, 2] = value                  # a second offender: the smallest triangle is named
    refused(MC.raw_desc(verts, faces), "triangle %d has a vertex index outside [0, 5)" % min(t, 5))


def test_bad_index_is_reported_before_any_non_finite_vertex():
    verts = TRI.copy()
    verts[0, 0] = np.inf                                # triangle 0 is not finite, triangle 2 has the bad index
    faces = FACES.copy()
    faces[2, 0] = 5
    refused(MC.raw_desc(verts, faces), "triangle 2 has a vertex index outside [0, 5)")


def test_non_finite_geometry():
    verts = TRI.copy()
    verts[4] = [np.nan, np.inf, -np.inf]
    assert MC.raw_call(MC.raw_desc(verts, FACES)[0]) == (0, "")            # unreferenced: the loader never sees it
    for bad in (np.nan, np.inf, -np.inf):
        verts = TRI.copy()
        verts[3, 1] = bad                               # referenced by triangles 1 and 2
        refused(MC.raw_desc(verts, FACES), "triangle 1 has a non-finite coordinate")
    soup = np.zeros((4, 9), np.float32)
    soup[2, 0] = soup[2, 3] = soup[3, 0] = soup[3, 3] = 3e38                # finite vertices, the sum overflows
    refused(MC.raw_desc(soup.reshape(-1, 3)),
            "triangle 2 has a non-finite centroid: the sum of its vertices overflows")
    soup[3, 8] = np.nan                                 # a later non-finite coordinate does not take precedence
    refused(MC.raw_desc(soup.reshape(-1, 3)), "triangle 2 has a non-finite centroid")
    soup[1, 8] = np.nan
    refused(MC.raw_desc(soup.reshape(-1, 3)), "triangle 1 has a non-finite coordinate")
    refused(MC.raw_desc(TRI, FACES, spheres=[[0, 0, 0, 1], [0, np.inf, 0, 1]]),
            "sphere 1 has a non-finite coordinate or radius")


def test_refusals_reach_python_as_rt_error():
    with pytest.raises(R.RtError, match=r"triangle 1 has a vertex index outside \[0, 5\)"):
        R.Scene.from_mesh(TRI, np.array([[0, 1, 2], [0, 5, 2]], np.int64))


# ---------------------------------------------------------------- Python argument checks

@pytest.mark.parametrize("kwargs,match", [
    (dict(vertices=TRI.astype(np.float64), faces=FACES), "vertices must be float32, not float64"),
    (dict(vertices=TRI[:, :2], faces=FACES), r"vertices must have shape \(n, 3\), not \(5, 2\)"),
    (dict(vertices=TRI[:4]), r"vertices of a soup \(faces=None\) must have shape"),
    (dict(vertices=np.zeros((2, 8), np.float32)), r"vertices of a soup \(faces=None\) must have shape"),
    (dict(vertices=TRI, faces=FACES.astype(np.float32)), "faces must be an integer array, not float32"),
    (dict(vertices=TRI, faces=FACES[:, :2]), r"faces must have shape \(n, 3\), not \(3, 2\)"),
    (dict(vertices=TRI, faces=FACES.astype(np.int64) + 2 ** 31), "faces has a value outside int32"),
    (dict(vertices=TRI, faces=FACES, materials=MC.MATERIALS[:, :11]), r"materials must have shape \(n, 12\)"),
    (dict(vertices=TRI, faces=FACES, materials=MC.MATERIALS.astype(np.float64)), "materials must be float32"),
    (dict(vertices=TRI, faces=FACES, materials=MC.MATERIALS, face_materials=[0, 1]),
     r"face_materials must have one entry per face \(3\), not 2"),
    (dict(vertices=TRI, faces=FACES, materials=MC.MATERIALS, face_materials=[0, 1, 70000]),
     "face_materials has a value outside uint16"),
    (dict(vertices=TRI, faces=FACES, materials=MC.MATERIALS, face_materials=[0.0, 1.0, 2.0]),
     "face_materials must be an integer array"),
    (dict(vertices=TRI, faces=FACES, spheres=np.zeros((2, 3), np.float32)), r"spheres must have shape \(n, 4\)"),
    (dict(vertices=TRI, faces=FACES, materials=MC.MATERIALS, spheres=np.zeros((2, 4), np.float32), sphere_materials=[0]),
     r"sphere_materials must have one entry per sphere \(2\), not 1"),
])
def test_python_argument_checks(kwargs, match):
    with pytest.raises(ValueError, match=match):
        R.Scene.from_mesh(**kwargs)


def test_python_accepts_the_documented_forms():
    soup = bvh_build_cases.vertices("size_65")
    want = R.Scene.from_mesh(soup).arrays()
    V, F = MC.indexed(soup)
    torch = pytest.importorskip("torch")
    for kw in (dict(vertices=soup.reshape(-1, 3, 3)), dict(vertices=soup.reshape(-1, 3)),
               dict(vertices=V, faces=F.astype(np.int64)), dict(vertices=torch.from_numpy(V), faces=torch.from_numpy(F))):
        got = R.Scene.from_mesh(**kw).arrays()
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)


# ---------------------------------------------------------------- downstream: the host twins, refit

def test_host_twins_on_a_from_mesh_scene(case_dir):
    d = cornell_description()
    want = MC.from_file(MC.write_canonical(d, os.path.join(case_dir, "twins.canonical.scene")))
    mesh = MC.from_mesh(d)
    pts = closest_point_scenes.sets("cornell")["uniform"][:64]
    got_cp, want_cp = mesh.closest_point(pts), want.closest_point(pts)
    assert all(got_cp[k].tobytes() == want_cp[k].tobytes() for k in want_cp)
    half = np.float32(0.1 * closest_point_scenes.extent(want.arrays())[2])
    boxes = np.ascontiguousarray(np.hstack([pts - half, pts + half]), np.float32)
    got_ov, want_ov = mesh.overlap_box(boxes, 8), want.overlap_box(boxes, 8)
    assert all(got_ov[k].tobytes() == want_ov[k].tobytes() for k in want_ov)
    assert got_ov["count"].max() > 0
    rays = np.ascontiguousarray(np.hstack([pts, np.tile(np.float32([0.3, -0.5, 0.8]), (64, 1))]), np.float32)
    got_mh, want_mh = mesh.multi_hit(rays, 4), want.multi_hit(rays, 4)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got_mh, want_mh))
    assert got_mh[2].max() > 0


def test_refit_leaves_the_face_index_alone():
    d = MC.case("size_257", True)
    s = MC.from_mesh(d)
    fi = s.face_index.copy()
    V2 = (d["vertices"] * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    s.refit(np.ascontiguousarray(V2[d["faces"][fi]].reshape(-1, 9)))           # the moving-geometry recipe
    assert np.array_equal(s.face_index, fi)
    assert s.arrays()["triangles"].tobytes() == records(V2[d["faces"][fi]].reshape(-1, 9)).tobytes()
