"""The virtual bounce-0 reorder (RTAMD_VREORDER; rt_render.hip: trace_kernel<.., VSLOT>, shade_rank_kernel,
fill_dead_kernel), bit for bit against the oracle and, counter for counter, against the moved reorder.

With the knob on, bounce 0 shades once in ray-id order and moves nothing; bounce 1 traces over the ray-id slots,
skipping the rays that ended at bounce 0, ranks every live slot to the reference's sorted position, shades with that
position as the seed, and scatters only the survivors of bounce 1.  RTAMD_VREORDER=1 forces that path for any scene
with triangles, so scenes of a few hundred rays reach it; unset, a scene past the fused reorder's size (teapot) takes
it on its own.  Every case checks the framebuffer against the oracle's and the counted work against the
RTAMD_VREORDER=0 render of the same scene.

45 rays per pixel are passes of 20, 20 and 5: at 24 x 16 the full passes are 30 whole 256-slot rounds and the last is
7.5.  Two bounces make bounce 1 the last one (no survivor is moved), three leave one plain reorder behind the new
kernel, six run the later bounces behind it.  The glow_* scenes carry kAccFlag through the in-place bounce 0 and the
new kernel's read-modify-write.
"""
import os

import numpy as np
import pytest

import edge_scenes
import oracle_lib as O
import refit_ref
import rtamd as R
import shade_scenes

pytestmark = pytest.mark.gpu

COUNTERS = ("live_segments", "nodes_popped", "internal_visits", "triangle_tests", "hits", "misses")
SHIPPED = ("cornell", "cornell_plus")
SHADE = ("glow_room", "glow_mixed", "glow_dark")
EDGE = ("deep", "big_leaf", "same_centroid")
SCENES = SHIPPED + SHADE + EDGE


def sky_only_scene():
    """Every ray ends at bounce 0 in the sky.  The one triangle stands behind the camera (the path serves scenes
    with triangles; none is ever hit), so the bounce-1 live count is 0."""
    return ("material white diffuse 0.8 0.8 0.8\n"
            "sky 0.6 0.7 0.9\n"
            "triangle white -1 -1 -5  1 -1 -5  0 1 -5\n"
            "camera position 0 0 0 forward 0 0 1 up 0 1 0 fov 40\n"
            "image 24 16 20 3 1\n")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return str(tmp_path_factory.mktemp("vreorder"))


@pytest.fixture(scope="module")
def paths(root):
    out = {name: os.path.join(R.ASSETS, name + ".scene") for name in SHIPPED + ("teapot",)}
    out.update(shade_scenes.write(root))
    out.update(edge_scenes.write(root))
    for name, text in (("same_centroid", refit_ref.same_centroid_scene(65)), ("sky_only", sky_only_scene())):
        out[name] = os.path.join(root, name + ".scene")
        with open(out[name], "w") as f:
            f.write(text)
    return out


def _asset_root(name, root):
    return R.ASSETS if name in SHIPPED + ("teapot",) else root


@pytest.fixture(scope="module")
def oracle(paths, root):
    """oracle(name, image) -> the sort-on framebuffer, rendered once per module and read-only."""
    cache = {}

    def get(name, image):
        if (name, image) not in cache:
            fb, _ = O.OracleScene(paths[name], asset_root=_asset_root(name, root), image=image).render(sort=True)
            fb.setflags(write=False)
            cache[(name, image)] = fb
        return cache[(name, image)]
    return get


def _diff(a, b):
    bad = a.view(np.uint32) != b.view(np.uint32)
    return "%d/%d values differ, first at %s: %r vs %r" % (int(bad.sum()), bad.size, np.flatnonzero(bad)[:4],
                                                          a[bad][:4], b[bad][:4])


def _render(paths, root, name, image):
    return R.render(R.Scene(paths[name], asset_root=_asset_root(name, root), image=image), sort=True, counters=True)


def _reports(capfd):
    """The renderers' setup reports (RTAMD_TIMING) printed since the last call: each names its bounce-0 reorder."""
    return [line for line in capfd.readouterr().err.splitlines() if line.startswith("rt_renderer init:")]


def _both_check(oracle, paths, root, monkeypatch, capfd, name, image, knob="1"):
    """The knob's render against the oracle's image and the RTAMD_VREORDER=0 render's counters (and that render
    against the oracle too: the yardstick of the counters is itself right).  The setup reports say which bounce-0
    reorder each render ran: the two renders must not be the same path twice."""
    ofb = oracle(name, image)
    monkeypatch.setenv("RTAMD_TIMING", "1")
    monkeypatch.setenv("RTAMD_VREORDER", "0")
    _reports(capfd)
    fb0, st0 = _render(paths, root, name, image)
    rep0 = _reports(capfd)
    assert len(rep0) == 1 and "bounce-0 reorder: moved" in rep0[0], rep0
    assert np.array_equal(fb0, ofb), _diff(fb0, ofb)
    if knob is None:
        monkeypatch.delenv("RTAMD_VREORDER")
    else:
        monkeypatch.setenv("RTAMD_VREORDER", knob)
    fb1, st1 = _render(paths, root, name, image)
    rep1 = _reports(capfd)
    assert len(rep1) == 1 and "bounce-0 reorder: virtual" in rep1[0], rep1
    assert fb1.shape == ofb.shape
    assert np.array_equal(fb1, ofb), _diff(fb1, ofb)
    for k in COUNTERS:
        assert st1[k] == st0[k], k
    return st1


@pytest.mark.parametrize("bounces", [2, 3, 6])
@pytest.mark.parametrize("name", SCENES)
def test_virtual_reorder_bitexact_and_same_work(oracle, paths, root, monkeypatch, capfd, name, bounces):
    _both_check(oracle, paths, root, monkeypatch, capfd, name, (24, 16, 45, bounces))


@pytest.mark.parametrize("name", ["glow_mixed", "cornell_plus"])
def test_plain_later_bounces_behind_the_virtual_reorder(oracle, paths, root, monkeypatch, capfd, name):
    """RTAMD_FUSED=0 under RTAMD_VREORDER=1: the later bounces in the form a big scene runs them (plain shade and
    scatter, the flag in rid)."""
    monkeypatch.setenv("RTAMD_FUSED", "0")
    _both_check(oracle, paths, root, monkeypatch, capfd, name, (24, 16, 45, 6))


@pytest.mark.parametrize("name", ["glow_mixed", "cornell"])
def test_short_last_tile(oracle, paths, root, monkeypatch, capfd, name):
    """23 x 15 pixels: passes of 6900 and 1725 rays, neither a multiple of 256, so the last round of the last tile
    is short in the trace over the slots and in the ranking."""
    _both_check(oracle, paths, root, monkeypatch, capfd, name, (23, 15, 45, 3))


@pytest.mark.parametrize("bounces", [2, 3])
def test_every_ray_ends_at_bounce_0(oracle, paths, root, monkeypatch, capfd, bounces):
    """live_1 == 0: the bounce-1 trace finds no live slot, the fill, histogram and scatter see an empty range."""
    st = _both_check(oracle, paths, root, monkeypatch, capfd, "sky_only", (24, 16, 45, bounces))
    assert st["live_segments"] == 24 * 16 * 45 and st["hits"] == 0


def test_renderer_reuse(oracle, paths, root, monkeypatch, capfd):
    """One renderer without counters (the kernels a plain render runs): the second pass alone, then the whole frame
    twice.  The bucket arrays, acc and the flags are per pass: nothing of an earlier run may be read back."""
    monkeypatch.setenv("RTAMD_TIMING", "1")
    monkeypatch.setenv("RTAMD_VREORDER", "1")
    image = (24, 16, 45, 6)
    ofb = oracle("glow_mixed", image)
    _reports(capfd)
    r = R.Renderer(R.Scene(paths["glow_mixed"], asset_root=root, image=image), sort=True)
    rep = _reports(capfd)
    assert len(rep) == 1 and "bounce-0 reorder: virtual" in rep[0], rep
    r.run(pass_begin=1, count=1)
    for _ in range(2):
        r.clear()
        r.run(pass_begin=0, count=-1)
        fb = r.framebuffer()
        assert np.array_equal(fb, ofb), _diff(fb, ofb)
    r.close()


@pytest.mark.parametrize("name,bounces", [("glow_mixed", 6), ("cornell_plus", 3)])
def test_renderer_reuse_counted(oracle, paths, root, monkeypatch, capfd, name, bounces):
    """The same reuse with the counters on: the second pass alone, then the whole frame twice, each whole-frame run's
    image against the oracle's and its counters against the RTAMD_VREORDER=0 render's of the same image.  A run's
    counts are its own: nothing carried over from the run before, no dead slot counted by the trace over the
    slots, no ray counted twice by the ranking kernel."""
    image = (24, 16, 45, bounces)
    ofb = oracle(name, image)
    monkeypatch.setenv("RTAMD_TIMING", "1")
    monkeypatch.setenv("RTAMD_VREORDER", "0")
    _reports(capfd)
    fb0, st0 = _render(paths, root, name, image)
    rep0 = _reports(capfd)
    assert len(rep0) == 1 and "bounce-0 reorder: moved" in rep0[0], rep0
    assert np.array_equal(fb0, ofb), _diff(fb0, ofb)
    monkeypatch.setenv("RTAMD_VREORDER", "1")
    r = R.Renderer(R.Scene(paths[name], asset_root=_asset_root(name, root), image=image), sort=True, counters=True)
    rep1 = _reports(capfd)
    assert len(rep1) == 1 and "bounce-0 reorder: virtual" in rep1[0], rep1
    first = r.run(pass_begin=1, count=1)
    assert 0 < first["live_segments"] < st0["live_segments"]
    for _ in range(2):
        r.clear()
        st = r.run(pass_begin=0, count=-1)
        fb = r.framebuffer()
        assert np.array_equal(fb, ofb), _diff(fb, ofb)
        for k in COUNTERS:
            assert st[k] == st0[k], k
    r.close()


def test_teapot_takes_the_virtual_reorder_by_default(oracle, paths, root, monkeypatch, capfd):
    """Knob and RTAMD_FUSED unset: a scene past the fused reorder's size takes the new path (the setup report names
    the bounce-0 reorder), and RTAMD_VREORDER=0 takes the moved one."""
    monkeypatch.delenv("RTAMD_FUSED", raising=False)
    _both_check(oracle, paths, root, monkeypatch, capfd, "teapot", (32, 18, 20, 3), knob=None)


def test_a_set_fused_knob_keeps_the_moved_reorder(oracle, paths, root, monkeypatch, capfd):
    """RTAMD_FUSED=2 names the fused replay at bounce 0: with RTAMD_VREORDER unset the big scene runs that, under
    the home index, not the virtual reorder."""
    monkeypatch.setenv("RTAMD_TIMING", "1")
    monkeypatch.setenv("RTAMD_FUSED", "2")
    monkeypatch.delenv("RTAMD_VREORDER", raising=False)
    image = (32, 18, 20, 3)
    _reports(capfd)
    fb, _ = _render(paths, root, "teapot", image)
    rep = _reports(capfd)
    assert len(rep) == 1 and "bounce-0 reorder: moved" in rep[0], rep
    ofb = oracle("teapot", image)
    assert np.array_equal(fb, ofb), _diff(fb, ofb)
