"""Scenes, rays, filters and yardstick answers shared by test_ray_filter_host.py (CPU) and test_gpu_ray_filter.py -- TEST
INFRASTRUCTURE ONLY.  Everything is computed once per process.

* scenes, ray sets (with twins' `through` and deep's constructed sets) and the oracle's closest hits (t_c, i_c) of the
  first 300 rays are multihit_scenes' (tests/multihit_scenes.py), by import.
* filters(scene, set, n): the filter runs over the first n rays.  Each run is a dict of the four members (None = not
  given) plus "masks" (the primitive mask words, or None).  A member's classes cycle over the rays, one class per ray,
  as test_gpu_query._tmax_classes does for tmax:
    none   nothing given;
    tmin   0, the float below t_c, t_c, the float above t_c, 2 t_c, NaN, +inf, -1 (None is the run "none");
    tmax   test_gpu_query._tmax_classes;
    skip   -1, i_c, the next ray's i_c, out of range;
    mask   with primitive masks from masks_from_materials, bit material % 32: all ones, 0, all but the bit of i_c's
           material, only that bit, seeded random;
    all    all four at once with the primitive masks: tmax's classes cycling, a seeded random class of each other
           member per ray.
* ref(scene): the yardstick's answers of every run of every set, over the first 300 rays (16 on teapot).
"""
import functools

import numpy as np

import multihit_scenes as M
import rtamd as R
from ray_filter_ref import RayFilterRef
from test_gpu_query import _tmax_classes

SCENES = M.SCENES
RUNS = ("none", "tmin", "tmax", "skip", "mask", "all")
N_REF = M.N_REF
MEMBERS = ("tmin", "tmax", "skip", "mask")


def n_ref(scene):
    return 16 if scene == "teapot" else N_REF


@functools.lru_cache(maxsize=None)
def prim_masks(scene):
    """The primitive mask words: bit material % 32."""
    dev = M.ctx(scene)["dev"]
    table = np.left_shift(np.uint32(1), (np.arange(dev.view.material_count) % 32).astype(np.uint32)).astype(np.uint32)
    return R.masks_from_materials(dev, table)


def _cycle(classes):
    """Class k of ray i with k = i mod the number of classes."""
    n = classes[0].shape[0]
    out = np.empty(n, classes[0].dtype)
    k = np.arange(n) % len(classes)
    for c, v in enumerate(classes):
        out[k == c] = v[k == c]
    return out


def _draw(classes, rng):
    """A seeded random class per ray."""
    n = classes[0].shape[0]
    out = np.empty(n, classes[0].dtype)
    k = rng.integers(0, len(classes), n)
    for c, v in enumerate(classes):
        out[k == c] = v[k == c]
    return out


def _tmin_list(t_c):
    n = t_c.shape[0]
    with np.errstate(all="ignore"):
        return [np.zeros(n, np.float32), np.nextafter(t_c, np.float32(-np.inf)), t_c.copy(),
                np.nextafter(t_c, np.float32(np.inf)), np.float32(2) * t_c, np.full(n, np.nan, np.float32),
                np.full(n, np.inf, np.float32), np.full(n, -1, np.float32)]


def _skip_list(i_c, prims):
    n = i_c.shape[0]
    return [np.full(n, -1, np.int32), i_c.astype(np.int32), np.roll(i_c, -1).astype(np.int32), np.full(n, prims + 5, np.int32)]


def _hit_bit(scene, i_c):
    """The mask bit of the material of each ray's closest primitive (bit 0 for a miss)."""
    mi = M.ctx(scene)["dev"].arrays()["material_indices"]
    mat = np.where(i_c >= 0, mi[np.maximum(i_c, 0)], 0).astype(np.uint32)
    return np.left_shift(np.uint32(1), mat % np.uint32(32)).astype(np.uint32)


def _mask_list(scene, i_c, rng):
    n = i_c.shape[0]
    bit = _hit_bit(scene, i_c)
    return [np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32), ~bit, bit,
            rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)]


@functools.lru_cache(maxsize=None)
def filters(scene, name, n):
    """{run: dict(tmin, tmax, skip, mask, masks)} over the first n (<= 300) rays of the set."""
    c = M.ctx(scene)
    t_c, i_c = c["t_c"][name][:n], c["i_c"][name][:n]
    prims = c["dev"].view.sphere_count + c["dev"].view.triangle_count
    rng = np.random.default_rng(4242)
    pm = prim_masks(scene)
    empty = dict(tmin=None, tmax=None, skip=None, mask=None, masks=None)
    runs = {"none": dict(empty), "tmin": dict(empty, tmin=_cycle(_tmin_list(t_c))),
            "tmax": dict(empty, tmax=np.ascontiguousarray(c["tm"][name][:n])),
            "skip": dict(empty, skip=_cycle(_skip_list(i_c, prims))),
            "mask": dict(empty, mask=_cycle(_mask_list(scene, i_c, rng)), masks=pm)}
    # all four at once: tmax's classes cycle as above, the other members' classes are drawn at random per ray
    runs["all"] = dict(tmin=_draw(_tmin_list(t_c), rng), tmax=_tmax_classes(t_c, rng), skip=_draw(_skip_list(i_c, prims), rng),
                       mask=_draw(_mask_list(scene, i_c, rng), rng), masks=pm)
    return runs


@functools.lru_cache(maxsize=None)
def _raw_cache(scene):
    return {}


@functools.lru_cache(maxsize=None)
def model(scene, masked):
    return RayFilterRef(M.ctx(scene)["dev"].arrays(), prim_masks(scene) if masked else None, _raw_cache(scene))


def members(run):
    return {k: run[k] for k in MEMBERS}


@functools.lru_cache(maxsize=None)
def ref(scene):
    """{set: {run: dict(rays, filter, closest=(t, index, ctr, life), anyhit=(occ, ctr, life))}} over the first
    n_ref(scene) rays of every set."""
    c = M.ctx(scene)
    n = n_ref(scene)
    out = {}
    for name, rays in c["sets"].items():
        r = np.ascontiguousarray(rays[:n])
        out[name] = {}
        for run, f in filters(scene, name, n).items():
            m = model(scene, f["masks"] is not None)
            out[name][run] = dict(rays=r, filter=f, closest=m.closest_batch(r, **members(f)),
                                  anyhit=m.anyhit_batch(r, **members(f)))
    return out


def tiled(f, n):
    """A run's members repeated to n rays (the GPU tests' 2,000-ray batches reuse the 300 classes)."""
    return {k: (None if f[k] is None else np.ascontiguousarray(np.resize(f[k], n))) for k in MEMBERS}
