"""The lean bounce-1 hand-over of the virtual reorder (rt_render.hip: shade_kernel<.., SLIM>, trace_kernel<.., VSLOT>,
shade_rank_kernel), bit for bit against the oracle.

A ray that survives bounce 0 is handed over as one 16-B record {d, t0} (+ material index and bucket byte); the bounce-1
trace recomputes the origin cam + t0 * primary_dir(ray) and writes a 4-B hit index per ray and, for the rays that hit,
the hit point o + closest * d, which shade_rank_kernel reads on those lanes only.  What can go wrong is in the scenes
(tests/lean_bounce1_scenes.py, tests/test_lean_bounce1_scenes.py): an origin that cancels in its last bits (far_cam),
hits and misses in the same waves (b1_mixed), sphere normals from the handed-over point (b1_spheres), terminations that
read acc before they write (slim_mix, glow_mixed), and the shipped cornell_plus and the sky map.

RTAMD_VREORDER=1 forces the path; every case also renders with the knob at 0 (the moved reorder, untouched) and checks
both framebuffers byte for byte and both renders' counted work against the oracle's.

Two bounces make bounce 1 the last one (every ray writes acc, hit or miss), three leave one plain reorder behind it,
six run the later bounces.  45 rays per pixel are passes of 20, 20 and 5: the longer pass's indices and hit points
stay behind the short pass's slots in the reused buffers.  23 x 15 pixels make every pass's last round and tile short.
"""
import os

import numpy as np
import pytest

import lean_bounce1_scenes
import oracle_lib as O
import rtamd as R
import shade_scenes
import slim_handover_scenes

pytestmark = pytest.mark.gpu

COUNTERS = ("live_segments", "nodes_popped", "internal_visits", "triangle_tests", "misses")
SHIPPED = ("cornell_plus",)
SCENES = tuple(lean_bounce1_scenes.NAMES) + ("slim_mix", "glow_mixed", "cornell_plus", "sky_16x8")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return str(tmp_path_factory.mktemp("lean"))


@pytest.fixture(scope="module")
def paths(root):
    out = {name: os.path.join(R.ASSETS, name + ".scene") for name in SHIPPED}
    out.update(shade_scenes.write(root))
    out.update(slim_handover_scenes.write(root))
    out.update(lean_bounce1_scenes.write(root))
    return out


def _asset_root(name, root):
    return R.ASSETS if name in SHIPPED else root


@pytest.fixture(scope="module")
def oracle(paths, root):
    """oracle(name, image) -> (sort-on framebuffer, stats), rendered once per module and read-only."""
    cache = {}

    def get(name, image):
        if (name, image) not in cache:
            fb, st = O.OracleScene(paths[name], asset_root=_asset_root(name, root), image=image).render(sort=True)
            fb.setflags(write=False)
            cache[(name, image)] = (fb, st)
        return cache[(name, image)]
    return get


def _diff(a, b):
    bad = a.view(np.uint32) != b.view(np.uint32)
    return "%d/%d values differ, first at %s: %r vs %r" % (int(bad.sum()), bad.size, np.flatnonzero(bad)[:4],
                                                          a[bad][:4], b[bad][:4])


def _reports(capfd):
    """The renderers' setup reports (RTAMD_TIMING) printed since the last call: each names its bounce-0 reorder."""
    return [line for line in capfd.readouterr().err.splitlines() if line.startswith("rt_renderer init:")]


def _check(oracle, paths, root, monkeypatch, capfd, name, image):
    ofb, ost = oracle(name, image)
    monkeypatch.setenv("RTAMD_TIMING", "1")
    for knob in ("1", "0"):
        monkeypatch.setenv("RTAMD_VREORDER", knob)
        _reports(capfd)
        fb, st = R.render(R.Scene(paths[name], asset_root=_asset_root(name, root), image=image), sort=True,
                          counters=True)
        rep = _reports(capfd)
        want = "bounce-0 reorder: virtual" if knob == "1" else "bounce-0 reorder: moved"
        assert len(rep) == 1 and want in rep[0], (knob, rep)
        assert fb.shape == ofb.shape
        assert fb.tobytes() == ofb.tobytes(), (knob, _diff(fb, ofb))
        for k in COUNTERS:
            assert st[k] == ost[k], (knob, k)
        assert st["hits"] == ost["hits_triangle"] + ost["hits_sphere"], knob


@pytest.mark.parametrize("bounces", [2, 3, 6])
@pytest.mark.parametrize("name", SCENES)
def test_lean_bounce1_bitexact_and_same_work(oracle, paths, root, monkeypatch, capfd, name, bounces):
    _check(oracle, paths, root, monkeypatch, capfd, name, (24, 16, 40, bounces))


@pytest.mark.parametrize("bounces", [2, 3, 6])
@pytest.mark.parametrize("name", ["b1_mixed", "far_cam"])
def test_last_pass_of_5_rays_per_pixel(oracle, paths, root, monkeypatch, capfd, name, bounces):
    """45 rays per pixel: passes of 20, 20 and 5 in the same buffers."""
    _check(oracle, paths, root, monkeypatch, capfd, name, (24, 16, 45, bounces))


@pytest.mark.parametrize("name", ["b1_mixed", "b1_spheres", "cornell_plus"])
def test_short_last_tile(oracle, paths, root, monkeypatch, capfd, name):
    """23 x 15 pixels: passes of 6900 and 1725 rays, neither a multiple of 256."""
    _check(oracle, paths, root, monkeypatch, capfd, name, (23, 15, 45, 3))


@pytest.mark.parametrize("name", ["b1_mixed", "b1_spheres"])
def test_renderer_reuse_without_counters(oracle, paths, root, monkeypatch, name):
    """The kernels a plain render runs (no counters), one renderer: the second pass alone, then the whole frame
    twice.  A slot that hit in one pass misses in another (40 % to 20 % of the bounce-1 rays hit): the hit point an
    earlier pass left at such a slot, and its index, may not be read back."""
    monkeypatch.setenv("RTAMD_VREORDER", "1")
    image = (24, 16, 45, 6)
    ofb, _ = oracle(name, image)
    r = R.Renderer(R.Scene(paths[name], asset_root=root, image=image), sort=True)
    r.run(pass_begin=1, count=1)
    for _ in range(2):
        r.clear()
        r.run(pass_begin=0, count=-1)
        fb = r.framebuffer()
        assert fb.tobytes() == ofb.tobytes(), _diff(fb, ofb)
    r.close()
