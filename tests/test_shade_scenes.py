"""CPU side of the synthetic shading scenes (tests/shade_scenes.py), no GPU.

* Witnesses, from the oracle's own counters: the scenes do what the GPU tests need them for (rays that
  receive a nonzero radiance term at every bounce and stay alive; sums of subnormals; misses next to sphere
  and triangle hits).  Without them an edit to a scene could leave the GPU tests vacuous.
* The product's CPU path (rt_cpu_render: the shared rt_device.h arithmetic on the host) equals the oracle's
  bit for bit on every scene, and the product loader builds the oracle's arrays.
* The sky lookup's texel index (row stride env_h, scene.cu:389-391) stays inside a map that is at least as
  wide as tall; a taller map is refused by the loader and by check_scene (here through rt_cpu_render).
"""
import numpy as np
import pytest

import oracle_lib as O
import rtamd as R
import shade_scenes

FLT_MIN = np.float32(1.1754944e-38)       # the smallest normal float32


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shade"))


@pytest.fixture(scope="module")
def paths(root):
    return shade_scenes.write(root)


@pytest.fixture(scope="module")
def oracle_renders(paths, root):
    """{(name, sort): (framebuffer, stats)} of the four glow scenes, rendered once."""
    out = {}
    for name in shade_scenes.GLOW:
        sc = O.OracleScene(paths[name], asset_root=root)
        for sort in (True, False):
            out[name, sort] = sc.render(sort=sort)
    return out


@pytest.mark.parametrize("sort", [True, False])
def test_glow_balls_every_ray_hits_at_every_bounce(oracle_renders, sort):
    """Every material has a nonzero emit component and nonzero albedos, and nothing misses: each ray gets a
    nonzero term at each of its 6 bounces and stays alive in between (the acc read-modify-write, 5 times)."""
    _, st = oracle_renders["glow_balls", sort]
    assert st["generated_rays"] == 24 * 16 * 40
    assert st["misses"] == 0
    assert st["hits_sphere"] == st["generated_rays"] * 6        # measured: 92160 of 92160
    assert st["hits_triangle"] == 0                             # the INLINE shade path's condition


@pytest.mark.parametrize("sort", [True, False])
def test_glow_room_nearly_every_ray_hits_at_every_bounce(oracle_renders, sort):
    """As glow_balls, with triangles; the few misses slip between two quads (measured: 92023 hits with the
    reorder, 91992 without, of 92160)."""
    _, st = oracle_renders["glow_room", sort]
    assert st["hits_triangle"] >= 0.99 * st["generated_rays"] * 6
    assert st["hits_sphere"] == 0


@pytest.mark.parametrize("sort", [True, False])
def test_glow_dark_is_all_subnormal(oracle_renders, sort):
    fb, _ = oracle_renders["glow_dark", sort]
    assert fb.size == 16 * 12 * 3
    assert (fb != 0).all()
    assert (np.abs(fb) < FLT_MIN).all()                          # measured: max 6.88e-39


@pytest.mark.parametrize("sort", [True, False])
def test_glow_mixed_reaches_sky_spheres_and_stays_finite(oracle_renders, sort):
    fb, st = oracle_renders["glow_mixed", sort]
    assert st["misses"] > 0 and st["hits_sphere"] > 0 and st["hits_triangle"] > 0   # measured: ~3100, ~25700, ~56700
    assert np.isfinite(fb).all()
    assert (fb < 0).any()                                        # the negative emitter shows


@pytest.mark.parametrize("name", shade_scenes.NAMES)
def test_cpu_path_bitexact(paths, root, name):
    ofb, _ = O.OracleScene(paths[name], asset_root=root).render_cpu_path()
    pfb, _ = R.cpu_render(R.Scene(paths[name], asset_root=root), threads=4)
    assert np.array_equal(ofb.view(np.uint32), pfb.view(np.uint32))


@pytest.mark.parametrize("name", shade_scenes.NAMES)
def test_loader_matches_oracle(paths, root, name):
    got = R.Scene(paths[name], asset_root=root).arrays()
    want = O.OracleScene(paths[name], asset_root=root).arrays()
    for k in ("materials", "spheres", "triangles", "material_indices", "bvh", "env"):
        assert got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def test_sky_maps_load_as_written(paths, root):
    """The loaded env array is the PFM's texels, row-major, for a non-square map too."""
    for w, h in shade_scenes.SKY_MAPS:
        env = R.Scene(paths["sky_%dx%d" % (w, h)], asset_root=root).arrays()["env"]
        want = (np.random.default_rng(3).random((h, w, 3)) * 4).astype(np.float32)
        assert 0 <= want.min() and want.max() < 4
        assert np.array_equal(env, want.reshape(-1, 3))


def _directions(n):
    rng = np.random.default_rng(5)
    d = rng.normal(size=(n, 3))
    d[: n // 4, rng.integers(0, 3)] = 0                          # a zero component
    d[n // 4: n // 3, 1] = 0
    d[n // 3: n // 3 + n // 20, 0:2] = 0                         # two: along +-z
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    axes = np.vstack([np.eye(3), -np.eye(3)])
    return np.ascontiguousarray(np.vstack([axes, d]), np.float32)


@pytest.mark.parametrize("w,h", [(16, 8), (5, 3), (7, 1), (8, 8), (1, 1)])
def test_env_texel_index_is_inside_a_wide_map(w, h):
    L = O.lib()
    dirs = _directions(100000)
    top = 0
    for d in dirs:
        i = L.orc_env_texel(O.ptr(d), w, h)
        assert 0 <= i < w * h, (d, i)
        top = max(top, i)
    assert top >= h * (h - 1)                # the last row (ty = h - 1, at stride h) is reached


def test_tall_sky_map_fails_to_load(tmp_path):
    shade_scenes.write_pfm(str(tmp_path / shade_scenes.pfm_name(3, 5)), 3, 5)
    p = str(tmp_path / "sky_3x5.scene")
    with open(p, "w") as f:
        f.write(shade_scenes.sky_scene(3, 5))
    with pytest.raises(R.RtError, match="row stride"):
        R.Scene(p, asset_root=str(tmp_path))
    # the same map lying on its side loads
    shade_scenes.write_pfm(str(tmp_path / shade_scenes.pfm_name(5, 3)), 5, 3)
    with open(p, "w") as f:
        f.write(shade_scenes.sky_scene(5, 3))
    assert R.Scene(p, asset_root=str(tmp_path)).view.environment_map_width == 5


def test_tall_sky_map_view_is_refused_by_cpu_render(paths, root):
    psc = R.Scene(paths["sky_5x3"], asset_root=root)
    want, _ = R.cpu_render(psc, threads=2)
    with shade_scenes.swapped_env(psc):
        assert (psc.view.environment_map_width, psc.view.environment_map_height) == (3, 5)
        with pytest.raises(R.RtError, match="row stride"):
            R.cpu_render(psc, threads=2)
    got, _ = R.cpu_render(psc, threads=2)                        # the view is whole again
    assert np.array_equal(got, want)
