"""CPU side of tests/slim_handover_scenes.py, no GPU: the scene holds what tests/test_gpu_slim_handover.py needs it
for, the product loader builds the oracle's arrays from it, and the product's CPU path renders it as the oracle does.
"""
import numpy as np
import pytest

import oracle_lib as O
import rtamd as R
import slim_handover_scenes as S

FLT_MIN = np.float32(1.1754944e-38)       # the smallest normal float32


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    return S.write(str(tmp_path_factory.mktemp("slim")))["slim_mix"]


def test_loader_matches_oracle(path):
    got = R.Scene(path).arrays()
    want = O.OracleScene(path).arrays()
    for k in ("materials", "spheres", "triangles", "material_indices", "bvh"):
        assert got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def test_materials_hold_the_edge_values(path):
    """Rows of 12 floats: diffuse, metallicity | specular, roughness | emit, ior, in the file's order."""
    m = np.asarray(R.Scene(path).arrays()["materials"], np.float32).reshape(-1, 12)
    tinyalb, subspec, negzero, neg, sub, half, pane, lamp, plain = m
    assert 0 < tinyalb[0] < FLT_MIN and tinyalb[0] == np.float32(S.SUBNORMAL_DIFFUSE)
    assert 0 < subspec[4] < FLT_MIN and subspec[3] == 1                    # always the specular albedo
    assert (negzero[8:11].view(np.uint32) == 0x80000000).all()             # -0: no radiance, whatever the sign bit
    assert neg[8] < 0 and 0 < sub[8] < FLT_MIN
    assert half[3] == 0.5 and (half[0:3] != half[4:7]).all()               # either albedo, and they differ
    assert pane[11] == 1.5 and (pane[0:3] != pane[4:7]).all()
    assert (lamp[0:3] == 0).all() and (lamp[4:7] == 0).all() and (lamp[8:11] > 0).all()   # ends where it hits
    assert (plain[8:11].view(np.uint32) == 0).all()


@pytest.mark.parametrize("sort", [True, False])
def test_oracle_reaches_spheres_triangles_and_ends_rays_early(path, sort):
    fb, st = O.OracleScene(path).render(sort=sort)
    rays = S.IMAGE[0] * S.IMAGE[1] * S.IMAGE[2]
    assert st["generated_rays"] == rays
    assert st["hits_sphere"] > 0 and st["hits_triangle"] > 0
    assert rays < st["live_segments"] < rays * S.IMAGE[3]                  # some rays end before the last bounce
    assert np.isfinite(fb).all() and (fb < 0).any()                        # the negative emitter shows


def test_cpu_path_bitexact(path):
    ofb, _ = O.OracleScene(path).render_cpu_path()
    pfb, _ = R.cpu_render(R.Scene(path), threads=4)
    assert np.array_equal(ofb.view(np.uint32), pfb.view(np.uint32))
