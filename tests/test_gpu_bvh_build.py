"""GPU binned-SAH build (csrc/bvh_build.hip) against the host build (the reference's recursion,
restated and pinned by tests/test_scene_parity.py): the node array, the triangle order and the
material-index order must be byte-identical, for every shipped scene, the edge scenes, and
random triangle soups full of coordinate ties and -0/+0 pairs (the reference's min/max keeps the
first of equal values, so the sign of a zero bound depends on the order of the triangles).

tests/bvh_build_cases.py adds the inputs that sit where the kernels change their code path: the three
launch regimes by node length and their tile and chunk edges, a chunked node that may not split (depth
limit, no_bvh), nodes with no axis to split on, a degenerate partition, zero costs, and a level that
mixes chunked, 1024-lane and one-wave nodes.  tests/test_bvh_build_cases.py certifies on the CPU that
each case reaches its path and that the host build there equals a numpy model and the oracle."""
import os

import numpy as np
import pytest

import bvh_build_cases
import edge_scenes
import rtamd as R

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "cornell_plus", "spheres", "teapot", "glass_teapot", "lamp_available"]


@pytest.fixture(scope="module")
def gpu():
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return 0


def _same(path, use_bvh=True):
    host = R.Scene(path, use_bvh=use_bvh)
    dev = R.Scene(path, use_bvh=use_bvh, bvh_device=0)
    a, b = host.arrays(), dev.arrays()
    for k in ("bvh", "triangles", "material_indices", "camera"):
        assert a[k].tobytes() == b[k].tobytes(), k
    return host, dev


@pytest.mark.parametrize("scene", SCENES)
def test_gpu_build_equals_host_build(gpu, scene):
    _same(os.path.join(R.ASSETS, scene + ".scene"))


def test_gpu_build_no_bvh(gpu):
    _same(os.path.join(R.ASSETS, "cornell.scene"), use_bvh=False)


def test_gpu_build_edge_scenes(gpu, tmp_path):
    for p in edge_scenes.write(str(tmp_path)).values():
        _same(p)


@pytest.mark.parametrize("seed,n", [(1, 3000), (2, 20000), (3, 777), (4, 90000)])   # 90000: chunked huge nodes
def test_gpu_build_random_soup_with_ties(gpu, tmp_path, seed, n):
    rng = np.random.default_rng(seed)
    vals = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0], np.float64)
    lines = [bvh_build_cases.HEADER]
    for i in range(n):
        if rng.random() < 0.5:
            v = rng.choice(vals, size=(3, 3))          # ties and signed zeros
        else:
            v = rng.normal(size=(3, 3)) * rng.choice([0.01, 1.0, 100.0])
        lines.append("triangle " + bvh_build_cases.MATERIALS[i % 5] + " " + " ".join(repr(float(x)) for x in v.ravel()) + "\n")
    lines.append("camera position 0 0 -10 forward 0 0 1 up 0 1 0 fov 40\nimage 16 16 1 1 1\n")
    p = tmp_path / ("soup%d.scene" % seed)
    p.write_text("".join(lines))
    host, _ = _same(str(p))
    assert host.view.bvh_node_count > 1


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("bvh_build_cases"))


@pytest.mark.parametrize("name", bvh_build_cases.names())
def test_gpu_build_cases(gpu, case_dir, name):
    _same(bvh_build_cases.write(name, case_dir))


def test_gpu_build_no_bvh_chunked_root(gpu, case_dir):
    """max_depth 0 on 32,769 triangles: a chunked root that may not split (box only, one leaf)."""
    host, _ = _same(bvh_build_cases.write("size_32769", case_dir), use_bvh=False)
    assert host.view.bvh_node_count == 1


def test_gpu_build_twice_in_one_process(gpu, case_dir):
    """Nothing is kept between builds; the scratch buffers are sized by each call."""
    path = bvh_build_cases.write("mixed_level", case_dir)
    small = bvh_build_cases.write("size_4097", case_dir)
    a = R.Scene(path, bvh_device=0).arrays()
    R.Scene(small, bvh_device=0)                       # a smaller build in between
    b = R.Scene(path, bvh_device=0).arrays()
    for k in ("bvh", "triangles", "material_indices", "camera"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_gpu_build_one_huge_coordinate(gpu, tmp_path):
    """One coordinate of 3e38 is finite, and so is its centroid: the load is defined (the root's area is inf,
    no cost is below it, one leaf), and the device build agrees with the host's."""
    p = tmp_path / "huge_coordinate.scene"
    t = ["0 0 0 1 0 0 0 1 0", "2 0 0 3 0 0 2 1 0", "4 0 1 5 0 0 4 1 0", "6 0 0 3e38 0 2 6 1 0", "8 1 0 9 0 0 8 1 3",
         "10 0 0 11 0 0 10 1 0"]
    p.write_text(bvh_build_cases.scene_text(["triangle %s %s\n" % (bvh_build_cases.MATERIALS[i % 5], v)
                                             for i, v in enumerate(t)]))
    host, _ = _same(str(p))
    assert host.view.bvh_node_count == 1


def test_gpu_build_refuses_non_finite_geometry(gpu, tmp_path):
    """rt_scene_load refuses a NaN or infinite coordinate before the device builder runs, as before the host's."""
    p = tmp_path / "bad.scene"
    for bad in ("nan", "inf", "-inf"):
        p.write_text(bvh_build_cases.scene_text(["triangle white 0 0 0 1 %s 0 0 1 0\n" % bad]))
        with pytest.raises(R.RtError, match="triangle 0 has a non-finite coordinate"):
            R.Scene(str(p), bvh_device=0)


def test_gpu_build_renders_identically(gpu):
    path = os.path.join(R.ASSETS, "teapot.scene")
    img = (64, 36, 20, 8)
    a, _ = R.render(R.Scene(path, image=img), sort=True)
    b, _ = R.render(R.Scene(path, image=img, bvh_device=0), sort=True)
    assert np.array_equal(a, b)


def test_cli_gpu_bvh_png_identical(gpu, tmp_path):
    import subprocess
    args = [R.CLI_PATH, "teapot.scene", "--image", "48", "32", "20", "6", "0.7"]
    a = subprocess.run(args + ["--out", str(tmp_path / "a.png")], cwd=R.ASSETS, capture_output=True, text=True)
    b = subprocess.run(args + ["--gpu-bvh", "--out", str(tmp_path / "b.png")], cwd=R.ASSETS, capture_output=True,
                       text=True)
    assert a.returncode == 0 and b.returncode == 0, a.stdout + b.stdout
    assert "Node count: 81311" in a.stdout and "Node count: 81311" in b.stdout
    assert open(tmp_path / "a.png", "rb").read() == open(tmp_path / "b.png", "rb").read()
