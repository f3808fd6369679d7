"""The slim bounce-0 hand-over of the virtual reorder (rt_render.hip: shade_kernel<.., SLIM>, trace_kernel<.., VSLOT>,
shade_rank_kernel), bit for bit against the oracle.

On that path a ray that survives bounce 0 is handed to bounce 1 as 27 bytes: {o, d}, the bounce-0 hit's material
index and, in bit 7 of its bucket byte, which albedo `scatter` multiplied into the throughput.  Bounce 1 rebuilds
T = 1 * albedo and the "acc[ray] holds radiance" flag has_radiance(0 + emit * 1) from the material row.  What can go
wrong is in the scenes: both albedo choices of a metal / diffuse split and of a dielectric (front and back face), a
bounce-0 sphere hit (the material comes through mat_idx[index]), emitters that scatter (the flag is set and acc is
read-modify-written later), emission that is negative, subnormal or -0 (no flag), subnormal albedo components, rays that
end at bounce 0 next to survivors (tests/slim_handover_scenes.py, tests/shade_scenes.py).

RTAMD_VREORDER=1 forces the path for any scene with triangles.  Every case renders with the knob at 1 and at 0 (the
moved reorder, whose kernels and layouts are untouched) and checks both framebuffers, byte for byte, and both
renders' counted work against the oracle's.  glow_balls has no triangles: the knob leaves it on the inline sphere
path, which must stay what it was.

24 x 16 pixels at 40 rays per pixel are two passes of 7680 rays, 30 whole 256-slot rounds each; 45 rays per pixel end
in a pass of 5 per pixel (1920 rays, 7.5 rounds); 23 x 15 makes every pass's last round short.  Two bounces make
bounce 1 the last one, three leave one plain reorder behind it, six run the later bounces.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import rtamd as R
import shade_scenes
import slim_handover_scenes

pytestmark = pytest.mark.gpu

COUNTERS = ("live_segments", "nodes_popped", "internal_visits", "triangle_tests", "misses")
SHIPPED = ("cornell_plus",)
SYNTHETIC = ("glow_balls", "glow_room", "glow_dark", "glow_mixed", "sky_16x8", "slim_mix")
SCENES = SHIPPED + SYNTHETIC
NO_TRIANGLES = ("glow_balls",)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return str(tmp_path_factory.mktemp("slim"))


@pytest.fixture(scope="module")
def paths(root):
    out = {name: os.path.join(R.ASSETS, name + ".scene") for name in SHIPPED}
    out.update(shade_scenes.write(root))
    out.update(slim_handover_scenes.write(root))
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
        virtual = knob == "1" and name not in NO_TRIANGLES
        want = "bounce-0 reorder: virtual" if virtual else "bounce-0 reorder: moved"
        assert len(rep) == 1 and want in rep[0], (knob, rep)
        assert fb.shape == ofb.shape
        assert fb.tobytes() == ofb.tobytes(), (knob, _diff(fb, ofb))
        for k in COUNTERS:
            assert st[k] == ost[k], (knob, k)
        assert st["hits"] == ost["hits_triangle"] + ost["hits_sphere"], knob


@pytest.mark.parametrize("bounces", [2, 3, 6])
@pytest.mark.parametrize("name", SCENES)
def test_slim_handover_bitexact_and_same_work(oracle, paths, root, monkeypatch, capfd, name, bounces):
    _check(oracle, paths, root, monkeypatch, capfd, name, (24, 16, 40, bounces))


@pytest.mark.parametrize("bounces", [2, 3, 6])
@pytest.mark.parametrize("name", ["slim_mix", "glow_mixed"])
def test_last_pass_of_5_rays_per_pixel(oracle, paths, root, monkeypatch, capfd, name, bounces):
    """45 rays per pixel: passes of 20, 20 and 5.  The material indices and bucket bytes of the longer pass before
    stay behind the short pass's slots in the same buffers."""
    _check(oracle, paths, root, monkeypatch, capfd, name, (24, 16, 45, bounces))


@pytest.mark.parametrize("name", ["slim_mix", "cornell_plus"])
def test_short_last_tile(oracle, paths, root, monkeypatch, capfd, name):
    """23 x 15 pixels: passes of 6900 and 1725 rays, neither a multiple of 256."""
    _check(oracle, paths, root, monkeypatch, capfd, name, (23, 15, 45, 3))


def test_renderer_reuse_without_counters(oracle, paths, root, monkeypatch):
    """The kernels a plain render runs (no counters), one renderer: the second pass alone, then the whole frame
    twice.  The hand-over arrays are per pass: nothing of an earlier run may be read back."""
    monkeypatch.setenv("RTAMD_VREORDER", "1")
    image = (24, 16, 45, 6)
    ofb, _ = oracle("slim_mix", image)
    r = R.Renderer(R.Scene(paths["slim_mix"], asset_root=root, image=image), sort=True)
    r.run(pass_begin=1, count=1)
    for _ in range(2):
        r.clear()
        r.run(pass_begin=0, count=-1)
        fb = r.framebuffer()
        assert fb.tobytes() == ofb.tobytes(), _diff(fb, ofb)
    r.close()
