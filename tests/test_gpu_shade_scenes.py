"""GPU parity on the synthetic shading scenes (tests/shade_scenes.py), through the C ABI, bit for bit
against the oracle (framebuffer and traversal / shading counters).

The glow_* scenes are the only ones in the suite in which a ray receives a nonzero radiance term and stays
alive (tests/test_shade_scenes.py has the witnesses), so they are what pins the renderer's acc[ray] /
kAccFlag scheme: the read-modify-write in shade_kernel, the flag's trip through sort_scatter_kernel
(RTAMD_FUSED=0) and its rebuild in sort_scatter_shade_kernel, the bounce-0 term left to the fused replay
under the home index (RTAMD_HOME), the inline sphere path, and `last` reading a flagged acc.  The oracle sums
`collected += emitted * transmitted` in hit order (scene.cu:383,417): the renderer's sums must come out in
that order.  glow_mixed adds the points of `scatter` no shipped material reaches, glow_dark float32
subnormals (the kernels must not flush them), and sky_WxH non-square environment maps.

Each render is two or three passes of 7680 rays: enough for rays to change waves and tiles in the reorder.
"""
import numpy as np
import pytest

import oracle_lib as O
import rtamd as R
import shade_scenes

pytestmark = pytest.mark.gpu

COUNTERS = ("live_segments", "nodes_popped", "internal_visits", "triangle_tests", "misses")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return str(tmp_path_factory.mktemp("shade"))


@pytest.fixture(scope="module")
def paths(root):
    return shade_scenes.write(root)


@pytest.fixture(scope="module")
def oracle(paths, root):
    """oracle(name, sort, image=None) -> (framebuffer, stats), each rendered once per module and read-only."""
    cache = {}

    def get(name, sort, image=None):
        key = (name, sort, image)
        if key not in cache:
            fb, st = O.OracleScene(paths[name], asset_root=root, image=image).render(sort=sort)
            fb.setflags(write=False)
            cache[key] = (fb, st)
        return cache[key]
    return get


def _diff(a, b):
    bad = a.view(np.uint32) != b.view(np.uint32)
    return "%d/%d values differ, first at %s: %r vs %r" % (int(bad.sum()), bad.size, np.flatnonzero(bad)[:4],
                                                          a[bad][:4], b[bad][:4])


def _check(gfb, gst, ofb, ost):
    assert gfb.shape == ofb.shape
    assert np.array_equal(gfb, ofb), _diff(gfb, ofb)
    for k in COUNTERS:
        assert gst[k] == ost[k], k
    assert gst["hits"] == ost["hits_triangle"] + ost["hits_sphere"]


def _render_check(oracle, paths, root, name, sort, image=None):
    ofb, ost = oracle(name, sort, image)
    gfb, gst = R.render(R.Scene(paths[name], asset_root=root, image=image), sort=sort, counters=True)
    _check(gfb, gst, ofb, ost)


# sort on with the radiance at the ray id or at the home index (RTAMD_HOME, read in Renderer::init), and sort off
@pytest.mark.parametrize("mode", ["sort-home0", "sort-home1", "unsorted"])
@pytest.mark.parametrize("fused", ["0", "1", "2", "3"])   # never, every bounce, bounce 0, bounces 0-1
@pytest.mark.parametrize("name", list(shade_scenes.GLOW))
def test_glow_fused_home_sort_variants_bitexact(oracle, paths, root, monkeypatch, name, fused, mode):
    """These scenes have under 4096 triangles, so the default is the fused replay at every bounce;
    RTAMD_FUSED=0 is what reaches rid[slot] = ray | kAccFlag in shade_kernel and the flag's trip through
    sort_scatter_kernel, 2 and 3 mix both within one pass."""
    monkeypatch.setenv("RTAMD_FUSED", fused)
    if mode != "unsorted":
        monkeypatch.setenv("RTAMD_HOME", mode[-1])
    _render_check(oracle, paths, root, name, mode != "unsorted")


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("bounces", [1, 2, 6])
@pytest.mark.parametrize("name", ["glow_room", "glow_balls"])
def test_glow_bounce_counts_and_partial_pass_bitexact(oracle, paths, root, name, bounces, sort):
    """1 bounce: `last` at bounce 0; 2: the home index is on and `last` at bounce 1 reads a flagged acc; 45 rays
    per pixel end in a pass of 5."""
    _render_check(oracle, paths, root, name, sort, image=(24, 16, 45, bounces))


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("inline", ["0", "1"])
def test_glow_balls_inline_and_traced_spheres_bitexact(oracle, paths, root, monkeypatch, inline, sort):
    """A scene of spheres only: the shade kernels' inline sphere loop, or the trace kernel's hits."""
    monkeypatch.setenv("RTAMD_FUSED", "1")
    monkeypatch.setenv("RTAMD_INLINE", inline)
    _render_check(oracle, paths, root, "glow_balls", sort)


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("name", shade_scenes.SKY)
def test_wide_sky_maps_bitexact(oracle, paths, root, name, sort):
    """Maps wider than tall (16x8, 5x3, 7x1): the lookup's row stride is the height, not the width."""
    _render_check(oracle, paths, root, name, sort)


def test_glow_room_pixel_tiles_with_sort_on_bitexact(oracle, paths):
    """Two tile owners with the per-bounce exchange (the plain shade / scatter pair with the flag in rid)."""
    from test_gpu_tiles import render_owners
    ofb, ost = oracle("glow_room", True)
    fb, sts = render_owners(paths["glow_room"], shade_scenes.GLOW_IMAGE, 4, 2, "host")
    assert np.array_equal(fb, ofb), _diff(fb, ofb)
    assert sum(s["live_segments"] for s in sts) == ost["live_segments"]


def test_glow_room_multi_device_path_bitexact(oracle, paths, root):
    """rt_render with a device list (rt_multi.hip: per-pass sums instead of the accumulating framebuffer)."""
    ofb, ost = oracle("glow_room", True)
    gfb, gst = R.render(R.Scene(paths["glow_room"], asset_root=root), sort=True, devices=[0])
    assert np.array_equal(gfb, ofb), _diff(gfb, ofb)
    assert gst["live_segments"] == ost["live_segments"]


@pytest.mark.parametrize("sort", [True, False])
def test_glow_mixed_renderer_reuse_bitexact(oracle, paths, root, sort):
    """One renderer: the second pass alone, then the whole frame twice.  acc and the flags are per pass: nothing
    of an earlier run's radiance may be read back (as test_renderer_reuse_bitexact, with flagged rays)."""
    ofb, _ = oracle("glow_mixed", sort)
    r = R.Renderer(R.Scene(paths["glow_mixed"], asset_root=root), sort=sort)
    r.run(pass_begin=1, count=1)
    for _ in range(2):
        r.clear()
        r.run(pass_begin=0, count=-1)
        fb = r.framebuffer()
        assert np.array_equal(fb, ofb), _diff(fb, ofb)
    r.close()


def test_tall_sky_map_view_is_refused_before_any_launch(paths, root):
    """An rt_scene whose map is taller than wide (the 5x3 scene's view with the two fields swapped) would make
    sky_color read past the map: every entry that uploads a scene refuses it in check_scene."""
    psc = R.Scene(paths["sky_5x3"], asset_root=root)
    rays = np.array([[0, 1.5, -4, 0, 0, 1]], np.float32)
    with shade_scenes.swapped_env(psc):
        with pytest.raises(R.RtError, match="row stride"):
            R.render(psc)
        with pytest.raises(R.RtError, match="row stride"):
            R.render(psc, devices=[0])
        with pytest.raises(R.RtError, match="row stride"):
            R.Renderer(psc)
        with pytest.raises(R.RtError, match="row stride"):
            R.trace_rays(psc, rays)
        with pytest.raises(R.RtError, match="row stride"):
            R.RayQuery(psc)
    t, idx, _ = R.trace_rays(psc, rays)          # the view is whole again
    assert idx[0] == 0 and t[0] > 0              # the mirror ball
