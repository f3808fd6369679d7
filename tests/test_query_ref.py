"""The any-hit yardstick (tests/anyhit_ref.py) against the oracle's closest hit, on the CPU.

With `closest` starting at 1e30 the closest hit (t_c, index) of a ray fixes two things about
occluded(ray, B) exactly: for B = 1e30, occluded <=> index >= 0; and occluded => t_c < B, so
for B = t_c, the float below t_c and 0.5 t_c the ray is never occluded.  (The converse fails just above
t_c -- an ancestor box's float entry distance can exceed the triangle's float t -- so nothing is asserted
there.)  Every ray must satisfy all four; no exceptions.
"""
import numpy as np
import pytest

import oracle_lib as O
from anyhit_ref import AnyHitRef
from test_gpu_trace_rays import _ray_sets

SETS = ("random", "axis_aligned", "vertex_origin", "vertex_origin_zero_component")


@pytest.mark.parametrize("scene", ["cornell", "cornell_plus", "spheres", "teapot"])
def test_anyhit_ref_agrees_with_closest_hit(scene):
    orc = O.OracleScene("%s/%s.scene" % (O.ASSETS, scene), image=(16, 16, 1, 1))
    ref = AnyHitRef(orc)
    sets = _ray_sets(orc, np.random.default_rng(1234), 300)
    hit_rays = 0
    for name in SETS:
        rays = sets[name]
        t_c, index, _ = orc.closest_hit(rays)
        assert not np.isnan(t_c).any()
        hit_rays += int((index >= 0).sum())
        mask, _ = ref.batch(rays, None)
        bad = np.nonzero(mask != (index >= 0))[0]
        assert bad.size == 0, "%s/%s B=1e30: %d rays differ, first %s" % (scene, name, bad.size, bad[:1])
        for what, B in (("t_c", t_c), ("below t_c", np.nextafter(t_c, np.float32(0))),
                        ("0.5 t_c", (np.float32(0.5) * t_c).astype(np.float32))):
            mask, _ = ref.batch(rays, B.astype(np.float32))
            assert not mask.any(), "%s/%s B=%s: %d rays occluded, first %s" % (
                scene, name, what, int(mask.sum()), np.nonzero(mask)[0][:1])
    assert hit_rays > 0
