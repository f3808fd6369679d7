"""CPU side of the lean bounce-1 scenes (tests/lean_bounce1_scenes.py), no GPU.

Witnesses from the oracle's own counters: each scene does what tests/test_gpu_lean_bounce1.py needs it for.  Bounce 0
of a render does not depend on the bounce count (the seeds are per bounce), so the counters of a 2-bounce render
minus those of a 1-bounce render are bounce 1's.
"""
import numpy as np
import pytest

import oracle_lib as O
import rtamd as R
import lean_bounce1_scenes
import shade_scenes
import slim_handover_scenes

RAYS = 24 * 16 * 40


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lean"))


@pytest.fixture(scope="module")
def paths(root):
    out = shade_scenes.write(root)
    out.update(slim_handover_scenes.write(root))
    out.update(lean_bounce1_scenes.write(root))
    return out


@pytest.fixture(scope="module")
def bounce1(paths, root):
    """bounce1(name) -> (bounce 0's stats, bounce 1's own counters), from 1- and 2-bounce oracle renders."""
    cache = {}

    def get(name):
        if name not in cache:
            st = [O.OracleScene(paths[name], asset_root=root, image=(24, 16, 40, b)).render(sort=True)[1] for b in (1, 2)]
            cache[name] = (st[0], {k: st[1][k] - st[0][k] for k in ("live_segments", "hits_triangle", "hits_sphere",
                                                                     "misses")})
        return cache[name]
    return get


def _share(b1):
    hits = b1["hits_triangle"] + b1["hits_sphere"]
    assert hits + b1["misses"] == b1["live_segments"]
    return hits / b1["live_segments"]


def test_far_cam_origin_cancels_and_rays_survive(paths, root, bounce1):
    v = R.Scene(paths["far_cam"], asset_root=root).view
    cam = v.camera_position
    assert np.linalg.norm([cam.x, cam.y, cam.z]) >= 3000
    tris = R.Scene(paths["far_cam"], asset_root=root).arrays()["triangles"]
    assert np.abs(tris).max() <= 4                               # the room: corners and edges of a few units, at the origin
    b0, b1 = bounce1("far_cam")
    assert b0["generated_rays"] == RAYS
    # rays beside the room's opening leave at bounce 0 (dead slots between the survivors); measured: 9474 of 15360
    assert 0.2 * RAYS < b0["misses"] < 0.8 * RAYS
    # every bounce-0 hit lies within the room, a few units from the origin, at t0 of about 5000: the survivors'
    # origins cam + t0 * d0 are 1000 times smaller than their terms; measured: 5886 survivors, 3695 hit again
    assert b1["live_segments"] > 0.3 * RAYS
    assert b1["hits_triangle"] > 1000 and b1["hits_sphere"] > 100 and b1["misses"] > 1000


def test_b1_mixed_hits_and_misses_share_the_waves(bounce1):
    """Measured: 10756 rays at bounce 1, 4696 hit (43.7 %), 6060 leave to the sky."""
    b0, b1 = bounce1("b1_mixed")
    assert b1["live_segments"] > 0.6 * RAYS
    assert 0.2 <= _share(b1) <= 0.8
    assert b0["misses"] > 1000                                   # dead slots in between


def test_b1_spheres_bounce1_rays_hit_spheres(bounce1):
    """Measured: 1463 bounce-1 sphere hits (and 2114 at bounce 0: the material comes through mat_idx[index])."""
    b0, b1 = bounce1("b1_spheres")
    assert b1["hits_sphere"] >= 1000
    assert b1["hits_triangle"] > 0 and b1["misses"] > 0
    assert b0["hits_sphere"] > 0


@pytest.mark.parametrize("name", ["slim_mix", "glow_mixed"])
def test_reused_scenes_have_scattering_emitters_at_bounce1(bounce1, name):
    """Nearly every ray hits at bounces 0 and 1 (measured shares at bounce 1: 99.9 % and 95.5 %), on emitters that
    scatter: acc_holds is set and a bounce-1 termination reads acc before it writes."""
    b0, b1 = bounce1(name)
    assert b0["misses"] == 0
    assert _share(b1) > 0.9 and b1["misses"] > 0
    assert b1["hits_sphere"] > 1000 and b1["hits_triangle"] > 1000


@pytest.mark.parametrize("name", lean_bounce1_scenes.NAMES)
def test_cpu_path_bitexact(paths, root, name):
    ofb, _ = O.OracleScene(paths[name], asset_root=root).render_cpu_path()
    pfb, _ = R.cpu_render(R.Scene(paths[name], asset_root=root), threads=4)
    assert np.array_equal(ofb.view(np.uint32), pfb.view(np.uint32))
