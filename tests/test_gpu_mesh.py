"""Scene.from_mesh on the device (rt_scene_from_mesh_device: csrc/mesh_ingest.hip's assemble and finalize kernels
around csrc/bvh_build.hip's level loop) against the host entry: arrays, view and face_index byte for
byte, the same refusals with the same messages, repeat builds, and resident queries on the result."""
import os

import numpy as np
import pytest

import bvh_build_cases
import mesh_cases as MC
import rtamd as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = ["size_1", "size_63", "size_64", "size_65", "size_257", "size_4097", "size_32769", "same_centroid_4097",
         "adjacent_floats_6", "denormal_range_6", "points_on_line", "mixed_level"]


@pytest.fixture(scope="module")
def gpu():
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return 0


_host = {}


def host_scene(name, mats, use_bvh=True):
    """The host entry's scene of a case, built once and left unchanged."""
    key = (name, mats, use_bvh)
    if key not in _host:
        _host[key] = MC.from_mesh(MC.case(name, False, with_materials=mats), use_bvh=use_bvh)
    return _host[key]


def on_device(desc):
    """The description with its triangle arrays as tensors on cuda:0."""
    d = dict(desc)
    for k in ("vertices", "faces", "face_materials"):
        if d.get(k) is not None:
            d[k] = torch.from_numpy(np.ascontiguousarray(d[k])).cuda()
    return d


@pytest.mark.parametrize("mats", [True, False], ids=["materials", "no_materials"])
@pytest.mark.parametrize("as_indexed", [False, True], ids=["soup", "indexed"])
@pytest.mark.parametrize("name", CASES)
def test_device_build_equals_host_build(gpu, name, as_indexed, mats):
    want = host_scene(name, mats)
    d = MC.case(name, as_indexed, with_materials=mats)
    assert MC.differences(MC.from_mesh(on_device(d)), want) == []           # device tensors
    assert MC.differences(MC.from_mesh(d, bvh_device=0), want) == []        # host arrays, device build


def test_device_build_no_bvh_chunked_root(gpu):
    want = host_scene("size_32769", True, use_bvh=False)
    for as_indexed in (False, True):
        d = MC.case("size_32769", as_indexed)
        got = MC.from_mesh(on_device(d), use_bvh=False)
        assert got.view.bvh_node_count == 1
        assert MC.differences(got, want) == []
        assert MC.differences(MC.from_mesh(d, bvh_device=0, use_bvh=False), want) == []


def test_index_tensor_is_a_slice_with_an_offset(gpu):
    d = MC.case("size_257", True)
    F = torch.from_numpy(d["faces"]).cuda()
    big = torch.full((F.shape[0] + 20, 3), 10 ** 9, dtype=torch.int32, device="cuda")
    big[7:7 + F.shape[0]] = F
    view = big[7:7 + F.shape[0]]
    assert view.storage_offset() == 21 and view.is_contiguous()
    got = MC.from_mesh(dict(on_device(d), faces=view))
    assert MC.differences(got, host_scene("size_257", True)) == []


def test_device_build_with_spheres_camera_and_int64_faces(gpu):
    d = MC.case("size_65", True)
    d["spheres"] = np.array([[0, 0, 0, 1], [50, -3, 2, 0.5]], np.float32)
    d["sphere_materials"] = [4, 1]
    want = MC.from_mesh(d)
    dd = on_device(d)
    dd["faces"] = dd["faces"].long()
    dd["face_materials"] = dd["face_materials"].view(torch.int16)
    assert MC.differences(MC.from_mesh(dd), want) == []


# ---------------------------------------------------------------- refusals

def message(desc, **kw):
    with pytest.raises(R.RtError) as e:
        MC.from_mesh(desc, **kw)
    assert str(e.value).startswith("rt error -1: ")
    return str(e.value)


def middle_slice(verts):
    """The vertices as a slice out of the middle of a larger allocation whose other rows are finite: a vertex index
    just outside the slice reads mapped, finite memory, so only the bounds check can refuse it."""
    n = verts.shape[0]
    big = torch.full((3 * n, 3), 0.25, dtype=torch.float32, device="cuda")
    big[n:2 * n] = torch.from_numpy(verts).cuda()
    return big[n:2 * n]


def check_refusal(desc, match):
    host = message(desc)
    assert match in host
    dd = on_device(desc)
    dd["vertices"] = middle_slice(np.ascontiguousarray(desc["vertices"]).reshape(-1, 3)).reshape(desc["vertices"].shape)
    assert message(dd) == host
    good = MC.case("size_65", True)                                          # the device is as good as before
    assert MC.differences(MC.from_mesh(on_device(good)), host_scene("size_65", True)) == []


@pytest.mark.parametrize("value", [-1, "vertex_count", -2 ** 31, 2 ** 31 - 1])
@pytest.mark.parametrize("where", ["first", "last"])
def test_device_refuses_a_bad_vertex_index(gpu, value, where):
    d = MC.case("size_4097", True)
    d["faces"] = d["faces"].copy()
    t = 0 if where == "first" else d["faces"].shape[0] - 1
    d["faces"][t, 2] = d["vertices"].shape[0] if value == "vertex_count" else value
    check_refusal(d, "triangle %d has a vertex index outside [0, %d)" % (t, d["vertices"].shape[0]))


def test_device_refuses_like_the_host(gpu):
    base = MC.case("size_4097", True)
    n, nv = base["faces"].shape[0], base["vertices"].shape[0]
    d = dict(base, face_materials=base["face_materials"].copy())
    d["face_materials"][1234] = 5
    check_refusal(d, "triangle 1234 has a material index outside the table of 5 materials")
    d["face_materials"][77] = 65535                                          # two offenders: the smaller index
    check_refusal(d, "triangle 77 has a material index outside")
    d = dict(base, faces=base["faces"].copy())
    d["faces"][3000, 0] = nv
    d["faces"][17, 1] = -5
    check_refusal(d, "triangle 17 has a vertex index outside")
    d = dict(base, vertices=base["vertices"].copy())
    v = int(base["faces"][2000, 1])
    d["vertices"][v, 2] = np.nan
    first = int(np.nonzero((base["faces"] == v).any(1))[0][0])
    check_refusal(d, "triangle %d has a non-finite coordinate" % first)
    soup = bvh_build_cases.vertices("size_4097").copy()
    soup[n - 1, 0] = soup[n - 1, 3] = soup[400, 1] = soup[400, 4] = 3e38
    check_refusal(dict(MC.case("size_4097"), vertices=soup),
                  "triangle 400 has a non-finite centroid: the sum of its vertices overflows")
    soup[399, 8] = -np.inf
    check_refusal(dict(MC.case("size_4097"), vertices=soup), "triangle 399 has a non-finite coordinate")
    # an unreferenced non-finite vertex is no error on either path
    d = dict(base, vertices=np.vstack([base["vertices"], np.full((1, 3), np.nan, np.float32)]))
    assert MC.differences(MC.from_mesh(on_device(d)), host_scene("size_4097", True)) == []


def test_python_checks_of_device_tensors(gpu):
    d = on_device(MC.case("size_65", True))
    with pytest.raises(ValueError, match="faces must be a tensor on the device of vertices, not ndarray"):
        R.Scene.from_mesh(d["vertices"], d["faces"].cpu().numpy())
    with pytest.raises(ValueError, match="vertices must be float32, not torch.float64"):
        R.Scene.from_mesh(d["vertices"].double(), d["faces"])
    with pytest.raises(ValueError, match="vertices must be contiguous"):
        R.Scene.from_mesh(d["vertices"].t().contiguous().t(), d["faces"])
    with pytest.raises(ValueError, match="faces must be contiguous"):
        R.Scene.from_mesh(d["vertices"], d["faces"].t().contiguous().t())
    with pytest.raises(ValueError, match="faces must be int32 or int64, not torch.int16"):
        R.Scene.from_mesh(d["vertices"], d["faces"].to(torch.int16))
    with pytest.raises(ValueError, match=r"faces must have shape \(n, 3\)"):
        R.Scene.from_mesh(d["vertices"], d["faces"].reshape(-1))
    with pytest.raises(ValueError, match="face_materials must be uint16 or int16, not torch.int32"):
        R.Scene.from_mesh(d["vertices"], d["faces"], MC.MATERIALS, d["face_materials"].to(torch.int32))
    with pytest.raises(ValueError, match="faces has a value outside int32"):
        R.Scene.from_mesh(d["vertices"], d["faces"].long() + 2 ** 31)
    with pytest.raises(ValueError, match="bvh_device 1 is not the tensors' device cuda:0"):
        R.Scene.from_mesh(d["vertices"], d["faces"], bvh_device=1)


# ---------------------------------------------------------------- repeat builds, streams

def test_device_build_twice_in_one_process(gpu):
    """Nothing is kept between builds; the scratch buffers are sized by each call."""
    big, small = on_device(MC.case("mixed_level", True)), on_device(MC.case("size_4097", True))
    a = MC.from_mesh(big)
    MC.from_mesh(small)                                  # a smaller build in between
    b = MC.from_mesh(big)
    assert MC.differences(a, b) == [] and MC.differences(a, host_scene("mixed_level", True)) == []


def test_inputs_made_on_another_stream_just_before_the_call(gpu):
    d = MC.case("size_32769", True)
    V0, F0 = torch.from_numpy(d["vertices"]).cuda(), torch.from_numpy(d["faces"]).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        V = V0
        for _ in range(20):                              # work the call has to wait for
            V = V * 1.0009765625 + 0.5
        F = F0.flip(0).contiguous()
        got = R.Scene.from_mesh(V, F, image=MC.IMAGE)
    want = R.Scene.from_mesh(V.cpu().numpy(), F.cpu().numpy(), image=MC.IMAGE)
    assert MC.differences(got, want) == []


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def teapot(gpu, tmp_path_factory):
    """teapot's triangles as a soup with the file's materials: (description, file-loaded query, from_mesh query)."""
    src = R.Scene(os.path.join(R.ASSETS, "teapot.scene"))
    a = src.arrays()
    d = dict(vertices=src.vertices(), materials=a["materials"], face_materials=a["material_indices"])
    path = MC.write_canonical(d, str(tmp_path_factory.mktemp("mesh_teapot") / "teapot.canonical.scene"))
    return d, R.RayQuery(MC.from_file(path), 0), R.RayQuery.from_mesh(**on_device(d), image=MC.IMAGE, exposure=MC.EXPOSURE)


def test_queries_on_a_from_mesh_teapot(teapot):
    d, filed, mesh = teapot
    assert MC.differences(mesh.scene, filed.scene) == []
    arr = filed.scene.arrays()
    lo, hi = arr["bvh"][0, 0:3], arr["bvh"][0, 3:6]
    rng = np.random.default_rng(20)
    n = 2000
    o = (lo + (hi - lo) * (rng.random((n, 3)) * 1.5 - 0.25)).astype(np.float32)
    t = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    rays = torch.from_numpy(np.ascontiguousarray(np.hstack([o, t - o]), np.float32)).cuda()
    pts = torch.from_numpy(o).cuda()
    half = np.float32(0.02) * (hi - lo)
    boxes = torch.from_numpy(np.ascontiguousarray(np.hstack([o - half, o + half]), np.float32)).cuda()
    (t1, i1), (t2, i2) = mesh.closest(rays), filed.closest(rays)
    assert torch.equal(t1, t2) and torch.equal(i1, i2) and int((i1 >= 0).sum()) > 100
    assert torch.equal(mesh.occluded(rays), filed.occluded(rays))
    c1, c2 = mesh.closest_point(pts), filed.closest_point(pts)
    assert all(torch.equal(c1[k], c2[k]) for k in c2)
    b1, b2 = mesh.overlap_box(boxes, 8), filed.overlap_box(boxes, 8)
    assert all(torch.equal(b1[k], b2[k]) for k in b2) and int(b1["count"].max()) > 0
    # answer indices map through face_index to the input faces: the hit triangle's record is that face's
    S = mesh.scene.view.sphere_count
    hit = i1.cpu().numpy()
    hit = hit[hit >= S]
    face = mesh.scene.face_index[hit - S]
    v = d["vertices"][face].reshape(-1, 3, 3)
    rec = np.hstack([v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]]).astype(np.float32)
    assert rec.tobytes() == np.ascontiguousarray(arr["triangles"][hit - S][:, 0:9]).tobytes()


def test_update_through_the_face_index(teapot):
    d, filed, _ = teapot
    V, F = MC.indexed(d["vertices"])
    mesh = R.RayQuery.from_mesh(torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda(), d["materials"],
                                torch.from_numpy(d["face_materials"]).cuda(), image=MC.IMAGE, exposure=MC.EXPOSURE)
    assert MC.differences(mesh.scene, filed.scene) == []
    V_new = torch.from_numpy(V).cuda() * 1.25 + 0.5
    Fl = torch.from_numpy(F).cuda().long()
    fi = torch.from_numpy(mesh.scene.face_index).cuda().long()
    mesh.update(V_new[Fl[fi]].reshape(-1, 9))                                # the documented recipe
    soup_new = V_new[Fl].reshape(-1, 9)                                      # the same moved vertices, input order
    filed.update(soup_new[torch.from_numpy(filed.scene.face_index).cuda().long()].contiguous())
    for g, w in zip(mesh.geometry(), filed.geometry()):
        assert g.tobytes() == w.tobytes()
    filed.update(torch.from_numpy(filed.scene.vertices()).cuda())            # the shared query goes back


def test_render_of_a_from_mesh_cornell(gpu, tmp_path):
    a = R.Scene(os.path.join(R.ASSETS, "cornell.scene")).arrays()
    t = a["triangles"]
    soup = np.ascontiguousarray(np.hstack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]]), np.float32)
    d = dict(vertices=soup, materials=a["materials"], face_materials=a["material_indices"],
             camera=((-278.0, 273.0, -800.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 37.0), sky=(0.1, 0.1, 0.2))
    img = (16, 16, 20, 3)
    want, _ = R.render(MC.from_file(MC.write_canonical(d, str(tmp_path / "cornell.scene")), image=img), sort=True)
    got, _ = R.render(MC.from_mesh(on_device(d), image=img), sort=True)
    assert np.array_equal(got, want) and float(np.abs(want).max()) > 0
