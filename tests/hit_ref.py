"""Yardstick for the hit records (rt_query_closest_hit, rt_scene_hit_records) -- TEST INFRASTRUCTURE ONLY.

HitRef restates the definition of include/rt_abi.h in vectorised numpy float32 over a scene's .arrays() (an
OracleScene's, a Scene's, or refit_ref.Arrays): every operation is an array operation on float32 arrays, so each is
rounded once and nothing is contracted; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  It takes (rays, t, index) and
returns every field, plus `t_re`: on triangle rows dot(e2, q) * f, the reference's own hit distance from the same f and
q that give u and v (scene.cu:166-183), which ties the restatement to the oracle's Möller-Trumbore.

same(a, b) is the comparison rule: element by element the bits are equal or both are NaN (the sign and payload of a
NaN that an operation produced differ between x86 and the GPU).
"""
import numpy as np

F32 = np.float32
FIELDS = ("t", "index", "uv", "normal", "position", "material", "front_face")


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def same(a, b):
    """True where two arrays of one dtype and shape agree: equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == F32:
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def differing_rows(a, b):
    """Indices of the rows (first axis) in which two arrays differ under same()."""
    ok = same(a, b)
    return np.nonzero(~ok.reshape(ok.shape[0], int(np.prod(ok.shape[1:]))).all(axis=1))[0]      # also for 0 rows


def _unit(v):
    v = np.asarray(v, F32)
    return (v / np.sqrt((v * v).sum(-1, keepdims=True)).astype(F32)).astype(F32)


def edge_rays(arrays, rng, n):
    """Seeded ray sets (n rays each) that the CPU and GPU tests share: origins exactly on a primitive's surface
    (a point p1 + e1/4 + e2/2 of a triangle with finite vertices, computed in float32; on scenes without
    triangles a point center + radius * unit of a sphere) with a random direction and with the direction along
    the surface normal, a NaN in each of the six ray components in turn, and a zero direction."""
    tri = np.ascontiguousarray(arrays["triangles"], F32).reshape(-1, 12)
    tri = tri[np.isfinite(tri[:, 0:9]).all(axis=1)]         # a zero-area triangle's normal is NaN: it stays
    sph = np.ascontiguousarray(arrays["spheres"], F32).reshape(-1, 4)
    rnd = _unit(rng.normal(size=(n, 3)))
    if tri.shape[0]:
        r = tri[rng.integers(0, tri.shape[0], n)]
        o = (r[:, 0:3] + F32(0.25) * r[:, 3:6] + F32(0.5) * r[:, 6:9]).astype(F32)
        nrm = r[:, 9:12]
    else:
        s = sph[rng.integers(0, sph.shape[0], n)]
        nrm = _unit(rng.normal(size=(n, 3)))
        o = (s[:, 0:3] + s[:, 3:4] * nrm).astype(F32)
    sign = np.where(np.arange(n) % 2 == 0, F32(1), F32(-1)).astype(F32)[:, None]
    sets = {"on_surface": np.hstack([o, rnd]), "on_surface_normal": np.hstack([o, sign * nrm])}
    lo, hi = o.min(0), o.max(0)
    base = np.hstack([(lo + rng.random((n, 3)) * (hi - lo + F32(1e-3))).astype(F32), _unit(rng.normal(size=(n, 3)))])
    nan = base.copy()
    nan[np.arange(n), np.arange(n) % 6] = np.nan
    zero = base.copy()
    zero[:, 3:6] = 0.0
    sets["nan_component"], sets["zero_direction"] = nan, zero
    return {k: np.ascontiguousarray(v, F32) for k, v in sets.items()}


class HitRef:
    def __init__(self, src):
        arr = src.arrays()
        self.spheres = np.ascontiguousarray(arr["spheres"], F32).reshape(-1, 4)
        self.tris = np.ascontiguousarray(arr["triangles"], F32).reshape(-1, 12)
        self.mat = np.ascontiguousarray(arr["material_indices"], np.uint16).reshape(-1)
        self.S = self.spheres.shape[0]

    def records(self, rays, t, index):
        rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
        t = np.ascontiguousarray(t, F32).reshape(-1)
        index = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = rays.shape[0]
        assert t.shape == (n,) and index.shape == (n,)
        o, d = rays[:, 0:3], rays[:, 3:6]
        out = dict(t=t.copy(), index=index.copy(), uv=np.zeros((n, 2), F32), normal=np.zeros((n, 3), F32),
                   position=np.zeros((n, 3), F32), material=np.full(n, -1, np.int32),
                   front_face=np.zeros(n, np.bool_), t_re=np.zeros(n, F32))
        hit = index >= 0
        tri = index >= self.S
        sph = hit & ~tri
        with np.errstate(all="ignore"):
            pos = o + t[:, None] * d                                # a multiply, then an add
            assert pos.dtype == F32
            out["position"][hit] = pos[hit]
            out["material"][hit] = self.mat[index[hit]].astype(np.int32)
            if tri.any():
                rec = self.tris[index[tri] - self.S]
                p1, e1, e2, nrm = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12]
                ot, dt = o[tri], d[tri]
                h = _cross(dt, e2)
                a = _dot(h, e1)
                f = F32(1.0) / a
                s = ot - p1
                u = _dot(s, h) * f
                q = _cross(s, e1)
                v = _dot(dt, q) * f
                assert u.dtype == F32 and v.dtype == F32 and q.dtype == F32 and f.dtype == F32
                out["uv"][tri] = np.stack([u, v], 1)
                out["normal"][tri] = nrm
                out["front_face"][tri] = _dot(nrm, dt) < 0
                out["t_re"][tri] = _dot(e2, q) * f
            if sph.any():
                sp = self.spheres[index[sph]]
                inv = F32(1.0) / sp[:, 3]
                nrm = inv[:, None] * (pos[sph] - sp[:, 0:3])
                assert nrm.dtype == F32
                out["normal"][sph] = nrm
                out["front_face"][sph] = _dot(nrm, d[sph]) < 0
        return out
