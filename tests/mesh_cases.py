"""Mesh descriptions for Scene.from_mesh and the canonical scene file that defines what from_mesh must
produce: rt_scene_from_mesh(description) == rt_scene_load(canonical file of the description), byte for byte.

A description is a dict of from_mesh's keyword arguments (vertices, faces, materials, face_materials, spheres,
sphere_materials, camera, sky).  Image and exposure are not part of the file: both sides get them as overrides
(IMAGE, EXPOSURE), which are what tests/bvh_build_cases.py's footer sets, so that bvh_build_cases.write(name, dir) is
a second, independently written file for case(name)'s description.
"""
import ctypes as C

import numpy as np

import bvh_build_cases
import rtamd as R

IMAGE, EXPOSURE = (16, 16, 1, 1), 1.0
# bvh_build_cases.HEADER's five materials as rt_material rows: diffuse, metallicity, specular, roughness, emit, ior
MATERIALS = np.array([[0.8, 0.8, 0.8, 0.2, 1, 1, 1, 0.3, 0, 0, 0, 0],
                      [0.5, 0.5, 0.5, 0, 1, 1, 1, 0, 0, 0, 0, 0],
                      [0.8, 0.1, 0.1, 0, 1, 1, 1, 0, 0, 0, 0, 0],
                      [0.1, 0.8, 0.1, 1, 1, 1, 1, 0.1, 0, 0, 0, 0],
                      [0.1, 0.1, 0.8, 0, 1, 1, 1, 0, 0, 0, 0, 0]], np.float32)
SKY = (0.6, 0.7, 0.9)
CAMERA = ((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 40.0)


def _f(x):
    return repr(float(x))


def soup_of(desc):
    """The description's triangles as (n, 9) float32 in input order, indexed or not."""
    v = np.asarray(desc["vertices"], np.float32)
    if desc.get("faces") is None:
        return v.reshape(-1, 9)
    return v[np.asarray(desc["faces"], np.int64)].reshape(-1, 9)


def canonical_text(desc):
    """The canonical scene file of a description (include/rt_abi.h): materials m<k> with all six parameters, sky,
    spheres, triangles in input order, camera; every float as repr(float(x)), which strtof reads back exactly."""
    out = []
    mats = desc.get("materials")
    if mats is None:
        out.append("material m0\n")
    else:
        for k, m in enumerate(np.asarray(mats, np.float32)):
            out.append("material m%d diffuse %s %s %s specular %s %s %s emit %s %s %s metallicity %s roughness %s ior %s\n"
                       % ((k,) + tuple(_f(x) for x in (m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10], m[3], m[7],
                                                        m[11]))))
    if desc.get("sky") is not None:
        out.append("sky %s %s %s\n" % tuple(_f(np.float32(x)) for x in desc["sky"]))
    sph = desc.get("spheres")
    if sph is not None:
        sm = desc.get("sphere_materials")
        for i, s in enumerate(np.asarray(sph, np.float32)):
            out.append("sphere m%d %s\n" % (0 if sm is None else int(sm[i]), " ".join(_f(x) for x in s)))
    fm = desc.get("face_materials")
    for i, t in enumerate(soup_of(desc)):
        out.append("triangle m%d %s\n" % (0 if fm is None else int(fm[i]), " ".join(_f(x) for x in t)))
    if desc.get("camera") is not None:
        p, f, u, fov = desc["camera"]
        out.append("camera position %s forward %s up %s fov %s\n"
                   % tuple([" ".join(_f(np.float32(x)) for x in v) for v in (p, f, u)] + [_f(np.float32(fov))]))
    return "".join(out)


def write_canonical(desc, path):
    with open(path, "w") as f:
        f.write(canonical_text(desc))
    return path


def indexed(soup, seed=5):
    """(n, 9) soup -> (V (V, 3) float32, F (n, 3) int32): vertex rows de-duplicated on their uint32 bit patterns (so
    -0 and +0 stay distinct vertices), then shuffled."""
    rows = np.ascontiguousarray(soup, np.float32).reshape(-1, 3)
    uniq, inverse = np.unique(rows.view(np.uint32), axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    perm = np.random.default_rng(seed).permutation(uniq.shape[0])
    where = np.empty_like(perm)
    where[perm] = np.arange(perm.shape[0])
    V = np.ascontiguousarray(uniq[perm]).view(np.float32)
    F = where[inverse].reshape(-1, 3).astype(np.int32)
    assert V[F].reshape(-1, 9).tobytes() == np.ascontiguousarray(soup, np.float32).tobytes()
    return V, F


def case(name, as_indexed=False, with_materials=True, camera=True, sky=True):
    """The description of bvh_build_cases case `name`: its triangles as a soup or an indexed mesh, its materials
    (i % 5 over MATERIALS), that module's camera and sky."""
    soup = bvh_build_cases.vertices(name)
    d = {}
    if as_indexed:
        d["vertices"], d["faces"] = indexed(soup)
    else:
        d["vertices"] = np.ascontiguousarray(soup, np.float32)
    if with_materials:
        d["materials"] = MATERIALS
        d["face_materials"] = bvh_build_cases.materials(name)
    if camera:
        d["camera"] = CAMERA
    if sky:
        d["sky"] = SKY
    return d


def from_mesh(desc, **kw):
    kw.setdefault("image", IMAGE)
    kw.setdefault("exposure", EXPOSURE)
    return R.Scene.from_mesh(**desc, **kw)


def from_file(path, **kw):
    kw.setdefault("image", IMAGE)
    kw.setdefault("exposure", EXPOSURE)
    return R.Scene(path, **kw)


def view_scalars(scene):
    """Every non-pointer field of the rt_scene view as bytes."""
    out = {}
    for name, typ in R.RtScene._fields_:
        if typ is R.P:
            continue
        val = getattr(scene.view, name)
        out[name] = bytes(val) if isinstance(val, C.Structure) else bytes(typ(val))
    return out


def differences(a, b, face_index=True):
    """Names of the arrays, view scalars (and face_index) on which two scenes differ as bytes."""
    bad = []
    x, y = a.arrays(), b.arrays()
    bad += [k for k in x if x[k].tobytes() != y[k].tobytes() or x[k].shape != y[k].shape]
    u, w = view_scalars(a), view_scalars(b)
    bad += [k for k in u if u[k] != w[k]]
    if face_index and a.face_index.tobytes() != b.face_index.tobytes():
        bad.append("face_index")
    return bad


def raw_desc(vertices=None, faces=None, face_materials=None, materials=None, spheres=None, sphere_materials=None,
             vertex_count=None, triangle_count=None, sphere_count=None, material_count=None):
    """An RtMeshDesc over numpy arrays with nothing checked, for the C entry's own refusals; counts default to the
    arrays'.  Returns (desc, keep): keep holds the arrays alive."""
    m = R.RtMeshDesc()
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return R._ptr(a)
    m.vertices = ptr(vertices, np.float32)
    m.indices = ptr(faces, np.int32)
    m.triangle_materials = ptr(face_materials, np.uint16)
    m.materials = ptr(materials, np.float32)
    m.spheres = ptr(spheres, np.float32)
    m.sphere_materials = ptr(sphere_materials, np.uint16)
    nv = 0 if vertices is None else np.asarray(vertices).size // 3
    m.vertex_count = nv if vertex_count is None else vertex_count
    nt = (nv // 3) if faces is None else np.asarray(faces).size // 3
    m.triangle_count = nt if triangle_count is None else triangle_count
    m.sphere_count = (0 if spheres is None else np.asarray(spheres).size // 4) if sphere_count is None else sphere_count
    m.material_count = (0 if materials is None else np.asarray(materials).size // 12) if material_count is None \
        else material_count
    return m, keep


def raw_call(m, image=IMAGE, bvh_device=-1, null_mesh=False, null_out=False):
    """rt_scene_from_mesh on a raw descriptor -> (rc, message); a scene that was made is freed."""
    L = R.lib()
    o = R.RtLoadOpts()
    L.rt_default_load_opts(C.byref(o))
    o.quiet = 1
    o.bvh_device = bvh_device
    if image is not None:
        o.image_override = 1
        o.width, o.height, o.ray_count, o.bounces = image
    h = R.P()
    L.rt_scene_from_mesh.argtypes = [R.P, R.P, R.P]
    rc = L.rt_scene_from_mesh(None if null_mesh else C.byref(m), C.byref(o), None if null_out else C.byref(h))
    msg = L.rt_last_error().decode() if rc else ""
    if h:
        L.rt_scene_free(h)
    return rc, msg
