"""ctypes host binding of librtamd.so (include/rt_abi.h) for Python callers.

This is plumbing for tests, the benchmark and the multi-GPU driver: every render call goes
through the C ABI into the HIP kernels.  There is no Python or CPU fallback for the GPU
path: if the library or a HIP device is missing, the calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
BUILD_DIR = os.path.join(PKG_DIR, "build")
# Up to 20 passes in flight on their own streams: HIP needs a hardware queue per stream.  Loading
# librtamd.so asks for 24 unless the variable is set (rt_abi.h); setting the same default here also
# covers a process where torch initialises HIP before the library loads.  A caller's value stands.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
LIB_PATH = os.environ.get("RTAMD_LIB") or os.path.join(BUILD_DIR, "librtamd.so")  # env: A/B builds only
# the same library with the multi-GPU test hooks (one-GPU loopback transport, failure injection):
# tests only, loaded beside the product library (test_lib())
TEST_LIB_PATH = os.path.join(BUILD_DIR, "librtamd_test.so")
CLI_PATH = os.path.join(BUILD_DIR, "raytracing")
HEADER = os.path.join(REPO, "include", "rt_abi.h")
ASSETS = os.path.join(REPO, "assets")


class RtError(RuntimeError):
    pass


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


P = C.c_void_p
I32 = C.c_int32


class RtScene(C.Structure):
    _fields_ = [("spheres", P), ("sphere_count", I32), ("triangles", P), ("triangle_count", I32),
                ("material_indices", P), ("materials", P), ("material_count", I32),
                ("bvh", P), ("bvh_node_count", I32), ("width", I32), ("height", I32),
                ("environment_map", P), ("environment_map_width", I32), ("environment_map_height", I32),
                ("camera_position", Vec3), ("forward", Vec3), ("up", Vec3),
                ("vertical_fov", C.c_float), ("exposure", C.c_float),
                ("min_coord", Vec3), ("inv_dimensions", Vec3),
                ("scaled_right", Vec3), ("scaled_up", Vec3), ("near_plane_top_left", Vec3),
                ("inv_width", C.c_float), ("inv_height", C.c_float),
                ("bounces", I32), ("ray_count", I32)]


class RtLoadOpts(C.Structure):
    _fields_ = [("use_bvh", I32), ("quiet", I32), ("asset_root", C.c_char_p), ("image_override", I32),
                ("width", I32), ("height", I32), ("ray_count", I32), ("bounces", I32),
                ("exposure_override", I32), ("exposure", C.c_float), ("bvh_device", I32)]


class RtCameraDesc(C.Structure):
    """rt_camera_desc: the `camera` line of a scene file."""
    _fields_ = [("position", Vec3), ("forward", Vec3), ("up", Vec3), ("vertical_fov_degrees", C.c_float)]


class RtMeshDesc(C.Structure):
    """rt_mesh_desc: a scene as arrays (rt_scene_from_mesh)."""
    _fields_ = [("vertices", P), ("vertex_count", I32), ("indices", P), ("triangle_count", I32),
                ("triangle_materials", P), ("spheres", P), ("sphere_count", I32), ("sphere_materials", P),
                ("materials", P), ("material_count", I32), ("camera", C.POINTER(RtCameraDesc)), ("sky", C.POINTER(Vec3))]


class RtOpts(C.Structure):
    _fields_ = [("sort", I32), ("device", I32), ("pass_begin", I32), ("pass_count", I32),
                ("pass_stride", I32), ("collect_counters", I32),
                ("tile_count", I32), ("tile_index", I32), ("tile_rows", I32),
                ("device_count", I32), ("device_ids", C.POINTER(I32)), ("shard_tiles", I32)]


# rt_exchange_fn: (user, bytes, n, hip_stream) -> 0 (pixel tiles with sort on, rt_renderer_set_exchange)
EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.c_void_p)


class RtStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("generated_rays", "live_segments", "sorted_items",
                                          "nodes_popped", "internal_visits", "triangle_tests",
                                          "sphere_tests", "hits", "misses", "hits_sphere",
                                          "dead_slots")] + \
               [("passes", C.c_uint32), ("reserved", C.c_uint32)] + \
               [(n, C.c_double) for n in ("render_ms", "kernel_ms", "process_ms", "sort_ms", "trace_ms")] + \
               [("trace_launches", C.c_uint64), ("exchange_ms", C.c_double)]

    def as_dict(self):
        return {n: (float(getattr(self, n)) if t is C.c_double else int(getattr(self, n)))
                for n, t in self._fields_ if n != "reserved"}


class RtHitOut(C.Structure):
    """rt_hit_out: one optional output pointer per hit-record field."""
    _fields_ = [(n, P) for n in ("t", "index", "uv", "normal", "position", "material", "front_face")]


HIT_FIELDS = tuple(n for n, _ in RtHitOut._fields_)
# field -> (shape after n, numpy dtype as the library writes it); front_face is returned as bool
HIT_SHAPES = {"t": ((), np.float32), "index": ((), np.int32), "uv": ((2,), np.float32), "normal": ((3,), np.float32),
              "position": ((3,), np.float32), "material": ((), np.int32), "front_face": ((), np.uint8)}


def _hit_fields(fields):
    """The requested hit-record fields as a tuple in HIT_FIELDS order; an unknown name raises ValueError."""
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    for k in names:
        if k not in HIT_SHAPES:
            raise ValueError("unknown hit-record field %r (known: %s)" % (k, ", ".join(HIT_FIELDS)))
    return tuple(k for k in HIT_FIELDS if k in names)


class RtMultiHitOut(C.Structure):
    """rt_multi_hit_out: t (n x k), index (n x k), count (n); every pointer optional."""
    _fields_ = [(n, P) for n in ("t", "index", "count")]


MULTI_HIT_MAX = 64   # RT_MULTI_HIT_MAX


def _multi_hit_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, not %s" % type(k).__name__)
    if not 1 <= int(k) <= MULTI_HIT_MAX:
        raise ValueError("k must be in 1..%d, not %d" % (MULTI_HIT_MAX, int(k)))
    return int(k)


class RtClosestPointOut(C.Structure):
    """rt_closest_point_out: distance (n), index (n), point (n x 3), uv (n x 2); every pointer optional."""
    _fields_ = [(n, P) for n in ("distance", "index", "point", "uv")]


CLOSEST_POINT_FIELDS = tuple(n for n, _ in RtClosestPointOut._fields_)
CLOSEST_POINT_SHAPES = {"distance": ((), np.float32), "index": ((), np.int32), "point": ((3,), np.float32),
                        "uv": ((2,), np.float32)}


def _closest_point_fields(fields):
    """The requested closest-point fields in CLOSEST_POINT_FIELDS order; an unknown name raises ValueError."""
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    for k in names:
        if k not in CLOSEST_POINT_SHAPES:
            raise ValueError("unknown closest-point field %r (known: %s)" % (k, ", ".join(CLOSEST_POINT_FIELDS)))
    return tuple(k for k in CLOSEST_POINT_FIELDS if k in names)


class RtNearestKOut(C.Structure):
    """rt_nearest_k_out: distance (n x k), index (n x k), point (n x k x 3), count (n); every pointer optional."""
    _fields_ = [(n, P) for n in ("distance", "index", "point", "count")]


NEAREST_K_MAX = 64   # RT_NEAREST_K_MAX
NEAREST_K_FIELDS = tuple(n for n, _ in RtNearestKOut._fields_)
NEAREST_K_DTYPES = {"distance": np.float32, "index": np.int32, "point": np.float32, "count": np.int32}


def _nearest_k_shape(field, n, k):
    return {"distance": (n, k), "index": (n, k), "point": (n, k, 3), "count": (n,)}[field]


def _nearest_k_args(k, fields):
    """k as an int in 1..NEAREST_K_MAX and the requested fields in NEAREST_K_FIELDS order, or ValueError."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, not %s" % type(k).__name__)
    if not 1 <= int(k) <= NEAREST_K_MAX:
        raise ValueError("k must be in 1..%d, not %d" % (NEAREST_K_MAX, int(k)))
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    for f in names:
        if f not in NEAREST_K_DTYPES:
            raise ValueError("unknown nearest-k field %r (known: %s)" % (f, ", ".join(NEAREST_K_FIELDS)))
    return int(k), tuple(f for f in NEAREST_K_FIELDS if f in names)


class RtOverlapOut(C.Structure):
    """rt_overlap_out: index (n x k) int32, count (n) int32, any (n) uint8; every pointer optional."""
    _fields_ = [(n, P) for n in ("index", "count", "any")]


OVERLAP_K_MAX = 64   # RT_OVERLAP_K_MAX
OVERLAP_FIELDS = tuple(n for n, _ in RtOverlapOut._fields_)
OVERLAP_DTYPES = {"index": np.int32, "count": np.int32, "any": np.uint8}


def _overlap_shape(field, n, k):
    return {"index": (n, k), "count": (n,), "any": (n,)}[field]


def _overlap_args(k, fields):
    """k as an int in 1..OVERLAP_K_MAX and the requested fields in OVERLAP_FIELDS order, or ValueError."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, not %s" % type(k).__name__)
    if not 1 <= int(k) <= OVERLAP_K_MAX:
        raise ValueError("k must be in 1..%d, not %d" % (OVERLAP_K_MAX, int(k)))
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    for f in names:
        if f not in OVERLAP_DTYPES:
            raise ValueError("unknown overlap field %r (known: %s)" % (f, ", ".join(OVERLAP_FIELDS)))
    return int(k), tuple(f for f in OVERLAP_FIELDS if f in names)


def _boxes_np(boxes):
    a = np.asarray(boxes)
    if a.dtype != np.float32:
        raise ValueError("boxes must be float32, not %s" % a.dtype)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError("boxes must have shape (n, 6), not %s" % (a.shape,))
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("boxes must be contiguous")
    return a


class RtRayFilter(C.Structure):
    """rt_ray_filter: tmin (n) float32, tmax (n) float32, skip (n) int32, mask (n) uint32; every pointer optional."""
    _fields_ = [(n, P) for n in ("tmin", "tmax", "skip", "mask")]


RAY_FILTER_DTYPES = {"tmin": np.float32, "tmax": np.float32, "skip": np.int32, "mask": np.uint32}


def _filter_np(n, **members):
    """The filter members given as numpy (None = not given): each a contiguous array of shape (n,) of its dtype, nothing
    converted.  Returns (RtRayFilter, the arrays to keep alive)."""
    keep = {}
    for name, dt in RAY_FILTER_DTYPES.items():
        v = members.get(name)
        if v is None:
            continue
        if _is_tensor(v):
            raise ValueError("%s must be a numpy array when rays is one" % name)
        a = np.asarray(v)
        if a.dtype != dt or a.shape != (n,) or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("%s must be a contiguous %s array of shape (n,)" % (name, np.dtype(dt).name))
        keep[name] = a
    return RtRayFilter(**{k: _ptr(a) for k, a in keep.items()}), keep


class RtHemisphereParams(C.Structure):
    """rt_hemisphere_params: samples, mode (0 cosine, 1 uniform), seed, point_offset."""
    _fields_ = [("samples", I32), ("mode", I32), ("seed", C.c_uint32), ("point_offset", C.c_uint32)]


class RtHemisphereOut(C.Structure):
    """rt_hemisphere_out: open_count (n) int32, openness (n) float32; every pointer optional."""
    _fields_ = [(n, P) for n in ("open_count", "openness")]


HEMISPHERE_MAX_SAMPLES = 4096   # RT_HEMISPHERE_MAX_SAMPLES
HEMISPHERE_MODES = {"cosine": 0, "uniform": 1}
HEMISPHERE_FIELDS = tuple(n for n, _ in RtHemisphereOut._fields_)
HEMISPHERE_DTYPES = {"open_count": np.int32, "openness": np.float32}


def _hemisphere_params(n, samples, mode, seed, point_offset):
    """RtHemisphereParams of the Python arguments, or ValueError: samples an int in 1..HEMISPHERE_MAX_SAMPLES with
    n * samples <= 2^31 - 1, mode a name of HEMISPHERE_MODES, seed and point_offset ints in 0..2^32 - 1."""
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)):
        raise ValueError("samples must be an integer, not %s" % type(samples).__name__)
    if not 1 <= int(samples) <= HEMISPHERE_MAX_SAMPLES:
        raise ValueError("samples must be in 1..%d, not %d" % (HEMISPHERE_MAX_SAMPLES, int(samples)))
    if mode not in HEMISPHERE_MODES:
        raise ValueError("unknown mode %r (known: %s)" % (mode, ", ".join(HEMISPHERE_MODES)))
    for name, v in (("seed", seed), ("point_offset", point_offset)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s must be an integer in 0..2^32 - 1, not %r" % (name, v))
    if n * int(samples) > 0x7FFFFFFF:
        raise ValueError("n * samples = %d does not fit int32" % (n * int(samples)))
    return RtHemisphereParams(int(samples), HEMISPHERE_MODES[mode], int(seed), int(point_offset))


def _hemisphere_fields(fields):
    """The requested outputs in HEMISPHERE_FIELDS order (at least one); an unknown name raises ValueError."""
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    for k in names:
        if k not in HEMISPHERE_DTYPES:
            raise ValueError("unknown hemisphere field %r (known: %s)" % (k, ", ".join(HEMISPHERE_FIELDS)))
    if not names:
        raise ValueError("fields must name at least one of %s" % ", ".join(HEMISPHERE_FIELDS))
    return tuple(k for k in HEMISPHERE_FIELDS if k in names)


def _frames_np(points, normals):
    """points and normals (n, 3) float32 numpy -> frames (n, 6) float32, contiguous."""
    p = _points_np(points)
    nm = np.asarray(normals)
    if nm.dtype != np.float32 or nm.shape != p.shape:
        raise ValueError("normals must be float32 of points' shape (n, 3), not %s %s" % (nm.dtype, nm.shape))
    return np.ascontiguousarray(np.hstack([p, nm]))


def hemisphere_rays(points, normals, samples, mode="cosine", seed=0, point_offset=0):
    """rt_hemisphere_rays: the n * samples sample rays (n * samples, 6) float32 that a hemisphere call with these
    arguments stands for, row i * samples + s = (points[i], direction of sample s); numpy, host only, no scene."""
    fr = _frames_np(points, normals)
    n = fr.shape[0]
    hp = _hemisphere_params(n, samples, mode, seed, point_offset)
    rays = np.zeros((n * hp.samples, 6), np.float32)
    f = lib().rt_hemisphere_rays
    f.argtypes = [P, I32, P, P]
    _check(f(_ptr(fr), n, C.byref(hp), _ptr(rays)))
    return rays


def _masks_np(masks, count):
    """Primitive mask words given as numpy: a contiguous uint32 array of sphere_count + triangle_count words."""
    a = np.asarray(masks)
    if a.dtype != np.uint32 or a.ndim != 1 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("masks must be a contiguous 1-D uint32 array, not %s %s" % (a.dtype, a.shape))
    if a.shape[0] != count:
        raise ValueError("masks must have sphere_count + triangle_count = %d words, not %d" % (count, a.shape[0]))
    return a


def masks_from_materials(scene, table):
    """Primitive mask words from materials: table[material_indices] as uint32, one word per primitive in the public
    numbering (spheres first).  table: one word per material of the scene (any integer array-like)."""
    t = np.asarray(table)
    if t.ndim != 1 or t.dtype.kind not in "iu":
        raise ValueError("table must be a 1-D integer array, not %s %s" % (t.dtype, t.shape))
    if t.shape[0] < scene.view.material_count:
        raise ValueError("table must have one word per material (%d), not %d" % (scene.view.material_count, t.shape[0]))
    if t.size and (t.min() < 0 or t.max() > 0xFFFFFFFF):
        raise ValueError("table words must fit uint32")
    return np.ascontiguousarray(t.astype(np.uint32)[scene.arrays()["material_indices"]])


def _points_np(points):
    a = np.asarray(points)
    if a.dtype != np.float32:
        raise ValueError("points must be float32, not %s" % a.dtype)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("points must have shape (n, 3), not %s" % (a.shape,))
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("points must be contiguous")
    return a


def _max_dist_np(max_dist, n):
    if max_dist is None:
        return None
    md = np.asarray(max_dist)
    if md.dtype != np.float32 or md.shape != (n,) or not md.flags["C_CONTIGUOUS"]:
        raise ValueError("max_dist must be a contiguous float32 array of shape (n,)")
    return md


def _tmax_np(tmax, n):
    if tmax is None:
        return None
    tm = np.asarray(tmax)
    if tm.dtype != np.float32 or tm.shape != (n,) or not tm.flags["C_CONTIGUOUS"]:
        raise ValueError("tmax must be a contiguous float32 array of shape (n,)")
    return tm


_lib = None


def build(jobs=8):
    subprocess.run(["make", "-s", "-j%d" % jobs, "-C", PKG_DIR], check=True)


_test_lib = None


def lib():
    """Load librtamd.so.  Raises if it has not been built: no fallback exists."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def test_lib():
    """librtamd_test.so (the test-hook build: RTAMD_MULTI_LOOPBACK, RTAMD_FAIL_AFTER_SETUP, RTAMD_TEST_SORT_GRID and
    the rtamd_test_* entry points to the reorder kernels), for tests.
    Scenes loaded through lib() can be passed to it: rt_scene is a plain host view."""
    global _test_lib
    if _test_lib is None:
        _test_lib = _load(TEST_LIB_PATH)
    return _test_lib


def _load(path):
    if not os.path.exists(path):
        raise RtError("%s is not built (run `make -C cuda-raytracer_amd` or "
                      "__graft_entry__.build())" % os.path.basename(path))
    L = C.CDLL(path)
    L.rt_last_error.restype = C.c_char_p
    L.rt_abi_version.restype = C.c_int
    L.rt_device_count.restype = C.c_int
    L.rt_default_opts.argtypes = [P]
    L.rt_default_load_opts.argtypes = [P]
    L.rt_scene_load.argtypes = [C.c_char_p, P, C.POINTER(P)]
    L.rt_scene_view.argtypes = [P]
    L.rt_scene_view.restype = C.POINTER(RtScene)
    L.rt_scene_bvh_ms.argtypes = [P]
    L.rt_scene_bvh_ms.restype = C.c_double
    L.rt_scene_free.argtypes = [P]
    L.rt_render.argtypes = [P, P, P, P]
    L.rt_renderer_create.argtypes = [P, P, C.POINTER(P)]
    L.rt_renderer_run.argtypes = [P, I32, I32, I32, P, P]
    L.rt_renderer_run_host.argtypes = [P, I32, I32, I32, P, P]
    L.rt_renderer_read_framebuffer.argtypes = [P, P]
    L.rt_renderer_clear.argtypes = [P]
    L.rt_renderer_set_counters.argtypes = [P, I32]
    L.rt_renderer_destroy.argtypes = [P]
    L.rt_trace_rays.argtypes = [P, P, P, I32, P, P, P]
    L.rt_bloom.argtypes = [P, I32, I32, C.c_float, I32, I32]
    L.rt_bloom_device.argtypes = [P, I32, I32, C.c_float, I32, I32]
    L.rt_tonemap.argtypes = [P, I32, I32, C.c_float, I32, P]
    L.rt_write_png.argtypes = [C.c_char_p, P, I32, I32]
    L.rt_cpu_render.argtypes = [P, P, I32, C.POINTER(C.c_double)]
    L.rt_multi_create.argtypes = [P, P, C.POINTER(P)]
    L.rt_multi_run.argtypes = [P, I32, P, P]
    L.rt_multi_read_framebuffer.argtypes = [P, P]
    L.rt_multi_set_event_timing.argtypes = [P, I32]
    L.rt_multi_set_counters.argtypes = [P, I32]
    L.rt_multi_ranks.argtypes = [P]
    L.rt_multi_destroy.argtypes = [P]
    return L


def _check(rc, L=None):
    if rc != 0:
        raise RtError("rt error %d: %s" % (rc, (L or lib()).rt_last_error().decode()))


def _ptr(a):
    return a.ctypes.data_as(P)


def warmup(device=0):
    """rt_device_warmup: HIP runtime, queues and code object initialised on `device`."""
    _check(lib().rt_device_warmup(device))


def device_count():
    return lib().rt_device_count()


def _mesh_np(x, what, dtype, shape_tail):
    """A from_mesh array given as numpy: dtype and shape (n,) + shape_tail checked, made contiguous, never converted."""
    a = np.asarray(x)
    if a.dtype != dtype:
        raise ValueError("%s must be %s, not %s" % (what, np.dtype(dtype).name, a.dtype))
    if a.ndim != len(shape_tail) + 1 or tuple(a.shape[1:]) != tuple(shape_tail):
        raise ValueError("%s must have shape (n%s), not %s" % (what, "".join(", %d" % s for s in shape_tail), a.shape))
    return np.ascontiguousarray(a)


def _mesh_indices_np(x, what, dtype, shape_tail):
    """Integer indices of any integer dtype, range-checked into `dtype` (int32 vertex indices, uint16 materials)."""
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError("%s must be an integer array, not %s" % (what, a.dtype))
    if a.ndim != len(shape_tail) + 1 or tuple(a.shape[1:]) != tuple(shape_tail):
        raise ValueError("%s must have shape (n%s), not %s" % (what, "".join(", %d" % s for s in shape_tail), a.shape))
    if a.dtype != dtype and a.size:
        info = np.iinfo(dtype)
        if int(a.min()) < info.min or int(a.max()) > info.max:
            raise ValueError("%s has a value outside %s" % (what, np.dtype(dtype).name))
    return np.ascontiguousarray(a, dtype)


def _soup_rows(shape, what="vertices"):
    """The triangle count of soup vertices of shape (F, 9), (F, 3, 3) or (3F, 3)."""
    if len(shape) == 2 and shape[1] == 9 or len(shape) == 3 and tuple(shape[1:]) == (3, 3):
        return int(shape[0])
    if len(shape) == 2 and shape[1] == 3 and shape[0] % 3 == 0:
        return int(shape[0]) // 3
    raise ValueError("%s of a soup (faces=None) must have shape (n, 9), (n, 3, 3) or (3n, 3), not %s" % (what, tuple(shape)))


def _mesh_arrays(tri, m, keep):
    """Scene.from_mesh's triangle arrays as numpy -> the descriptor's host pointers."""
    v, f, fm = tri["vertices"], tri["faces"], tri["face_materials"]
    v = np.asarray(v)
    if v.dtype != np.float32:
        raise ValueError("vertices must be float32, not %s" % v.dtype)
    if f is None:
        n = _soup_rows(v.shape)
        v = np.ascontiguousarray(v).reshape(-1, 3)
    else:
        v = _mesh_np(v, "vertices", np.float32, (3,))
        f = _mesh_indices_np(f, "faces", np.int32, (3,))
        n = f.shape[0]
        m.indices = _ptr(f)
    m.vertices, m.vertex_count, m.triangle_count = _ptr(v), v.shape[0], n
    if fm is not None:
        fm = _mesh_indices_np(fm, "face_materials", np.uint16, ())
        if fm.shape[0] != n:
            raise ValueError("face_materials must have one entry per face (%d), not %d" % (n, fm.shape[0]))
        m.triangle_materials = _ptr(fm)
    keep.extend([v, f, fm])


def _mesh_tensors(tri, on_gpu, m, keep):
    """Scene.from_mesh's triangle arrays as torch tensors on one GPU -> the descriptor's device pointers; returns
    the device index.  Nothing is copied except an int64 index tensor, which is range-checked and narrowed."""
    import torch
    given = [k for k, x in tri.items() if x is not None]
    for k in given:
        if k not in on_gpu:
            raise ValueError("%s must be a tensor on the device of %s, not %s" % (k, on_gpu[0], type(tri[k]).__name__))
    dev = tri[on_gpu[0]].device
    for k in given:
        x = tri[k]
        if x.device.type != "cuda" or x.device != dev:
            raise ValueError("%s must be on %s, not %s" % (k, dev, x.device))
    v, f, fm = tri["vertices"], tri["faces"], tri["face_materials"]
    if v is None:
        raise ValueError("vertices must be given")
    if v.dtype != torch.float32:
        raise ValueError("vertices must be float32, not %s" % v.dtype)
    if not v.is_contiguous():
        raise ValueError("vertices must be contiguous")
    if f is None:
        n = _soup_rows(tuple(v.shape))
        vcount = 3 * n
    else:
        if v.dim() != 2 or v.shape[1] != 3:
            raise ValueError("vertices must have shape (n, 3), not %s" % (tuple(v.shape),))
        vcount = int(v.shape[0])
        if f.dtype not in (torch.int32, torch.int64):
            raise ValueError("faces must be int32 or int64, not %s" % f.dtype)
        if f.dim() != 2 or f.shape[1] != 3:
            raise ValueError("faces must have shape (n, 3), not %s" % (tuple(f.shape),))
        if not f.is_contiguous():
            raise ValueError("faces must be contiguous")
        if f.dtype == torch.int64:
            if f.numel() and (int(f.min()) < -2 ** 31 or int(f.max()) > 2 ** 31 - 1):
                raise ValueError("faces has a value outside int32")
            f = f.to(torch.int32)
        n = int(f.shape[0])
        m.indices = P(f.data_ptr()) if n else None
    m.vertices, m.vertex_count, m.triangle_count = (P(v.data_ptr()) if vcount else None), vcount, n
    if fm is not None:
        ok = [torch.int16] + ([torch.uint16] if hasattr(torch, "uint16") else [])
        if fm.dtype not in ok:
            raise ValueError("face_materials must be uint16 or int16, not %s" % fm.dtype)
        if fm.dim() != 1 or int(fm.shape[0]) != n:
            raise ValueError("face_materials must have shape (%d,), not %s" % (n, tuple(fm.shape)))
        if not fm.is_contiguous():
            raise ValueError("face_materials must be contiguous")
        m.triangle_materials = P(fm.data_ptr()) if n else None
    keep.extend([v, f, fm])
    return dev.index if dev.index is not None else torch.cuda.current_device()


class Scene:
    """A scene loaded by the product loader (rt_scene_load), or made from arrays by from_mesh."""

    def __init__(self, path, use_bvh=True, asset_root=ASSETS, image=None, exposure=None, quiet=True,
                 bvh_device=-1):
        """bvh_device >= 0 builds the BVH on that GPU (same arrays as the host build)."""
        L = lib()
        o = RtLoadOpts()
        L.rt_default_load_opts(C.byref(o))
        o.use_bvh = int(use_bvh)
        o.bvh_device = int(bvh_device)
        o.quiet = int(quiet)
        self._root = asset_root.encode() if asset_root else None
        o.asset_root = self._root
        if image is not None:
            o.image_override = 1
            o.width, o.height, o.ray_count, o.bounces = [int(v) for v in image]
        if exposure is not None:
            o.exposure_override = 1
            o.exposure = float(exposure)
        h = P()
        _check(L.rt_scene_load(path.encode(), C.byref(o), C.byref(h)))
        self.h = h
        self.view = L.rt_scene_view(h).contents

    @classmethod
    def from_mesh(cls, vertices, faces=None, materials=None, face_materials=None, spheres=None, sphere_materials=None,
                  camera=None, sky=None, image=None, exposure=None, use_bvh=True, bvh_device=-1):
        """rt_scene_from_mesh / rt_scene_from_mesh_device: the scene of a mesh held in arrays, byte for
        byte what Scene(path) makes of the description's canonical scene file.

        vertices  (V, 3) float32; with faces=None a soup: (F, 9), (F, 3, 3) or (3F, 3), triangle i = rows 3i..3i+2.
        faces     (F, 3) int32; int64 is accepted and range-checked in the conversion.
        materials (M, 12) float32 rows laid out like arrays()["materials"]; None = the loader's default material.
        face_materials (F,), sphere_materials (S,) integers below M (None = all 0); spheres (S, 4) float32.
        camera    (position, forward, up, fov_degrees) or None; sky (r, g, b) or None.
        image     (width, height, spp, bounces) and exposure as Scene's.

        numpy arrays and CPU tensors take the host entry (bvh_device >= 0 builds the BVH on that GPU).  If vertices,
        faces or face_materials is a torch tensor on a GPU, all of them must be contiguous tensors on that one device
        (float32; int32 or int64; uint16 or int16) and the device entry reads them in place, after synchronising
        torch.cuda.current_stream(device); a bvh_device that is given must be that device.  Either way the result
        is a host-owned Scene.

        The two recipes a mesh user needs: an answer index i >= S (S = the sphere count) of any query is input
        face `scene.face_index[i - S]`; and moving geometry goes to a RayQuery as
        `q.update(V_new[F[scene.face_index]].reshape(-1, 9))` (V_new (V, 3), F (F, 3) long: plain indexing, numpy
        or torch on the device)."""
        L = lib()
        o = RtLoadOpts()
        L.rt_default_load_opts(C.byref(o))
        o.use_bvh = int(use_bvh)
        o.quiet = 1
        if image is not None:
            o.image_override = 1
            o.width, o.height, o.ray_count, o.bounces = [int(v) for v in image]
        if exposure is not None:
            o.exposure_override = 1
            o.exposure = float(exposure)
        m = RtMeshDesc()
        keep = []                                       # what the descriptor points into, alive until the call returns
        tri = {"vertices": vertices, "faces": faces, "face_materials": face_materials}
        tri = {k: (v.numpy() if _is_tensor(v) and v.device.type == "cpu" else v) for k, v in tri.items()}
        on_gpu = [k for k, v in tri.items() if _is_tensor(v)]
        stream = None
        if on_gpu:
            dev = _mesh_tensors(tri, on_gpu, m, keep)
            if int(bvh_device) >= 0 and int(bvh_device) != dev:
                raise ValueError("bvh_device %d is not the tensors' device cuda:%d" % (int(bvh_device), dev))
            o.bvh_device = dev
            import torch
            stream = torch.cuda.current_stream(dev).cuda_stream
        else:
            o.bvh_device = int(bvh_device)
            _mesh_arrays(tri, m, keep)
        if materials is not None:
            a = _mesh_np(materials, "materials", np.float32, (12,))
            m.materials, m.material_count = _ptr(a), a.shape[0]
            keep.append(a)
        if spheres is not None:
            a = _mesh_np(spheres, "spheres", np.float32, (4,))
            m.spheres, m.sphere_count = _ptr(a), a.shape[0]
            keep.append(a)
        if sphere_materials is not None:
            a = _mesh_indices_np(sphere_materials, "sphere_materials", np.uint16, ())
            if spheres is None or a.shape[0] != m.sphere_count:
                raise ValueError("sphere_materials must have one entry per sphere (%d), not %d"
                                 % (m.sphere_count, a.shape[0]))
            m.sphere_materials = _ptr(a)
            keep.append(a)
        if camera is not None:
            pos, fwd, up, fov = camera
            cam = RtCameraDesc(Vec3(*[float(x) for x in pos]), Vec3(*[float(x) for x in fwd]),
                               Vec3(*[float(x) for x in up]), float(fov))
            m.camera = C.pointer(cam)
            keep.append(cam)
        if sky is not None:
            sk = Vec3(*[float(x) for x in sky])
            m.sky = C.pointer(sk)
            keep.append(sk)
        h = P()
        if on_gpu:
            L.rt_scene_from_mesh_device.argtypes = [P, P, P, C.POINTER(P)]
            _check(L.rt_scene_from_mesh_device(C.byref(m), C.byref(o), P(stream) if stream else None, C.byref(h)))
        else:
            L.rt_scene_from_mesh.argtypes = [P, P, C.POINTER(P)]
            _check(L.rt_scene_from_mesh(C.byref(m), C.byref(o), C.byref(h)))
        self = cls.__new__(cls)
        self._root = None
        self.h = h
        self.view = L.rt_scene_view(h).contents
        return self

    def __del__(self):
        if getattr(self, "h", None):
            lib().rt_scene_free(self.h)
            self.h = None

    @property
    def face_index(self):
        """rt_scene_face_index: numpy int32 (triangle_count,); entry j is the input index of scene triangle j (answer
        index sphere_count + j of every query): the face given to from_mesh, or the triangle's position in the file."""
        L = lib()
        L.rt_scene_face_index.argtypes = [P, C.POINTER(C.POINTER(I32)), C.POINTER(I32)]
        p, n = C.POINTER(I32)(), I32()
        _check(L.rt_scene_face_index(self.h, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.int32)
        return np.ctypeslib.as_array(p, shape=(n.value,)).astype(np.int32, copy=True)

    @property
    def ptr(self):
        return lib().rt_scene_view(self.h)

    @property
    def width(self):
        return self.view.width

    @property
    def height(self):
        return self.view.height

    @property
    def pixels(self):
        return self.view.width * self.view.height

    @property
    def passes(self):
        return (self.view.ray_count + 19) // 20

    @property
    def bvh_ms(self):
        return lib().rt_scene_bvh_ms(self.h)

    def vertices(self):
        """The triangles' vertices, (n, 9) float32 {a.xyz, b.xyz, c.xyz} in the scene's triangle order,
        reconstructed from the records as p1, p1 + p2p1, p1 + p3p1: not necessarily the file's floats
        (b - a + a need not be b).  This is what a caller deforms and hands to refit / RayQuery.update."""
        t = self.arrays()["triangles"]
        return np.ascontiguousarray(np.hstack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]]), np.float32)

    def refit(self, vertices):
        """rt_scene_refit: new vertices (numpy (n, 9) float32, contiguous, the scene's triangle order)
        under the frozen BVH topology; triangles, node bounds and the reorder-key bounds are rewritten in
        place.  Objects created from the scene earlier keep their own device copies."""
        a = _vertices_np(vertices)
        f = lib().rt_scene_refit
        f.argtypes = [P, P, I32]
        _check(f(self.h, _ptr(a), a.shape[0]))

    def hit_records(self, rays, t, index, fields=HIT_FIELDS):
        """rt_scene_hit_records: the hit records of given closest hits on this host scene, no GPU:
        rays (n, 6) float32, t (n,) float32 and index (n,) int32 as closest / trace_rays return them, all numpy
        and contiguous.  Returns a dict of the requested fields ("t" and "index" are the arguments' copies)."""
        names = _hit_fields(fields)
        a = RayQuery._rays_np(rays)
        n = a.shape[0]
        tt, ii = np.asarray(t), np.asarray(index)
        if tt.dtype != np.float32 or tt.shape != (n,) or not tt.flags["C_CONTIGUOUS"]:
            raise ValueError("t must be a contiguous float32 array of shape (n,)")
        if ii.dtype != np.int32 or ii.shape != (n,) or not ii.flags["C_CONTIGUOUS"]:
            raise ValueError("index must be a contiguous int32 array of shape (n,)")
        out = {k: np.zeros((n,) + HIT_SHAPES[k][0], HIT_SHAPES[k][1]) for k in names if k not in ("t", "index")}
        ho = RtHitOut(**{k: _ptr(v) for k, v in out.items()})
        f = lib().rt_scene_hit_records
        f.argtypes = [P, P, P, P, I32, P]
        _check(f(self.ptr, _ptr(a), _ptr(tt), _ptr(ii), n, C.byref(ho)))
        if "t" in names:
            out["t"] = tt.copy()
        if "index" in names:
            out["index"] = ii.copy()
        if "front_face" in out:
            out["front_face"] = out["front_face"].view(np.bool_)
        return {k: out[k] for k in names}

    def multi_hit(self, rays, k, tmax=None):
        """rt_scene_multi_hit: the host twin of RayQuery.multi_hit, no GPU: rays (n, 6) float32 and
        tmax None or (n,) float32, numpy and contiguous.  Returns (t (n, k) float32, index (n, k) int32,
        count (n,) int32), bit for bit what the device call writes."""
        k = _multi_hit_k(k)
        a = RayQuery._rays_np(rays)
        n = a.shape[0]
        tm = _tmax_np(tmax, n)
        t, idx, cnt = np.zeros((n, k), np.float32), np.zeros((n, k), np.int32), np.zeros(n, np.int32)
        mo = RtMultiHitOut(_ptr(t), _ptr(idx), _ptr(cnt))
        f = lib().rt_scene_multi_hit
        f.argtypes = [P, P, P, I32, I32, P]
        _check(f(self.ptr, _ptr(a), _ptr(tm) if tm is not None else None, n, k, C.byref(mo)))
        return t, idx, cnt

    def closest_point(self, points, max_dist=None, fields=CLOSEST_POINT_FIELDS):
        """rt_scene_closest_point: the host twin of RayQuery.closest_point, no GPU: points (n, 3) float32
        and max_dist None or (n,) float32, numpy and contiguous.  Returns a dict of the requested fields, bit for
        bit what the device call writes."""
        names = _closest_point_fields(fields)
        a = _points_np(points)
        n = a.shape[0]
        md = _max_dist_np(max_dist, n)
        out = {k: np.zeros((n,) + CLOSEST_POINT_SHAPES[k][0], CLOSEST_POINT_SHAPES[k][1]) for k in names}
        co = RtClosestPointOut(**{k: _ptr(v) for k, v in out.items()})
        f = lib().rt_scene_closest_point
        f.argtypes = [P, P, P, I32, P]
        _check(f(self.ptr, _ptr(a), _ptr(md) if md is not None else None, n, C.byref(co)))
        return out

    def nearest_k(self, points, k, max_dist=None, fields=NEAREST_K_FIELDS):
        """rt_scene_nearest_k: the host twin of RayQuery.nearest_k, no GPU: points (n, 3) float32 and
        max_dist None or (n,) float32, numpy and contiguous.  Returns a dict of the requested fields, bit for bit what
        the device call writes."""
        k, names = _nearest_k_args(k, fields)
        a = _points_np(points)
        n = a.shape[0]
        md = _max_dist_np(max_dist, n)
        out = {f: np.zeros(_nearest_k_shape(f, n, k), NEAREST_K_DTYPES[f]) for f in names}
        no = RtNearestKOut(**{f: _ptr(v) for f, v in out.items()})
        f = lib().rt_scene_nearest_k
        f.argtypes = [P, P, P, I32, I32, P]
        _check(f(self.ptr, _ptr(a), _ptr(md) if md is not None else None, n, k, C.byref(no)))
        return out

    def overlap_box(self, boxes, k, fields=("index", "count")):
        """rt_scene_overlap_box: the host twin of RayQuery.overlap_box, no GPU: boxes (n, 6) float32
        {lo.xyz, hi.xyz}, numpy and contiguous.  Returns a dict of the requested fields, bit for bit what the device
        call writes."""
        k, names = _overlap_args(k, fields)
        a = _boxes_np(boxes)
        n = a.shape[0]
        out = {f: np.zeros(_overlap_shape(f, n, k), OVERLAP_DTYPES[f]) for f in names}
        oo = RtOverlapOut(**{f: _ptr(v) for f, v in out.items()})
        f = lib().rt_scene_overlap_box
        f.argtypes = [P, P, I32, I32, P]
        _check(f(self.ptr, _ptr(a), n, k, C.byref(oo)))
        return out

    def signed_distance(self, points, direction=(0.5773503, 0.5773503, 0.5773503)):
        """The host twin of RayQuery.signed_distance (numpy only): the same composition of closest_point and the
        count-only multi_hit on this host scene, no GPU."""
        return _signed_distance(self, points, direction)

    def _filtered_args(self, rays, tmin, tmax, skip, mask, masks):
        a = RayQuery._rays_np(rays)
        n = a.shape[0]
        rf, keep = _filter_np(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        m = None if masks is None else _masks_np(masks, self.view.sphere_count + self.view.triangle_count)
        return a, n, rf, keep, m

    def closest_filtered(self, rays, tmin=None, tmax=None, skip=None, mask=None, fields=("t", "index"), masks=None,
                         stats=False):
        """rt_scene_closest_filtered: the host twin of RayQuery.closest_filtered, no GPU: rays (n, 6)
        float32, the filter members None or (n,) arrays (tmin, tmax float32, skip int32, mask uint32) and masks None
        or sphere_count + triangle_count uint32 words, numpy and contiguous.  Returns a dict of the requested hit-record
        fields, bit for bit what the device call writes (the fields past t and index through hit_records); with
        stats=True a pair (dict, the walk's counters as a dict)."""
        names = _hit_fields(fields)
        a, n, rf, keep, m = self._filtered_args(rays, tmin, tmax, skip, mask, masks)
        t, idx = np.zeros(n, np.float32), np.zeros(n, np.int32)
        st = RtStats()
        f = lib().rt_scene_closest_filtered
        f.argtypes = [P, P, P, P, I32, P, P, P]
        _check(f(self.ptr, _ptr(m) if m is not None else None, _ptr(a), C.byref(rf), n, _ptr(t), _ptr(idx), C.byref(st)))
        out = self.hit_records(a, t, idx, names) if set(names) - {"t", "index"} else {k: {"t": t, "index": idx}[k] for k in names}
        return (out, st.as_dict()) if stats else out

    def occluded_filtered(self, rays, tmin=None, tmax=None, skip=None, mask=None, masks=None, stats=False):
        """rt_scene_occluded_filtered: the host twin of RayQuery.occluded_filtered, no GPU; arguments as
        closest_filtered's.  Returns a bool mask; with stats=True a pair (mask, the walk's counters as a dict)."""
        a, n, rf, keep, m = self._filtered_args(rays, tmin, tmax, skip, mask, masks)
        occ = np.zeros(n, np.uint8)
        st = RtStats()
        f = lib().rt_scene_occluded_filtered
        f.argtypes = [P, P, P, P, I32, P, P]
        _check(f(self.ptr, _ptr(m) if m is not None else None, _ptr(a), C.byref(rf), n, _ptr(occ), C.byref(st)))
        return (occ.view(np.bool_), st.as_dict()) if stats else occ.view(np.bool_)

    def hemisphere(self, points, normals, samples, mode="cosine", seed=0, point_offset=0, tmin=None, tmax=None, skip=None,
                   mask=None, fields=HEMISPHERE_FIELDS, masks=None, stats=False):
        """rt_scene_hemisphere: the host twin of RayQuery.hemisphere, no GPU: points and normals (n, 3)
        float32, the filter members None or (n,) arrays, one row per point, and masks None or sphere_count +
        triangle_count uint32 words, numpy and contiguous.  Returns a dict of the requested fields, bit for bit what
        the device call writes; with stats=True a pair (dict, the walks' counters summed over all n * samples rays)."""
        names = _hemisphere_fields(fields)
        fr = _frames_np(points, normals)
        n = fr.shape[0]
        hp = _hemisphere_params(n, samples, mode, seed, point_offset)
        rf, keep = _filter_np(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        m = None if masks is None else _masks_np(masks, self.view.sphere_count + self.view.triangle_count)
        out = {k: np.zeros(n, HEMISPHERE_DTYPES[k]) for k in names}
        ho = RtHemisphereOut(**{k: _ptr(v) for k, v in out.items()})
        st = RtStats()
        f = lib().rt_scene_hemisphere
        f.argtypes = [P, P, P, P, I32, P, P, P]
        _check(f(self.ptr, _ptr(m) if m is not None else None, _ptr(fr), C.byref(rf), n, C.byref(hp), C.byref(ho), C.byref(st)))
        return (out, st.as_dict()) if stats else out

    def arrays(self):
        v = self.view

        def arr(p, n, cols, dt=np.float32):
            if n == 0:
                return np.zeros((0, cols) if cols else 0, dt)
            itemsize = np.dtype(dt).itemsize * (cols or 1)
            buf = (C.c_char * (n * itemsize)).from_address(p)
            a = np.frombuffer(buf, dtype=dt).copy()
            return a.reshape(n, cols) if cols else a
        cam = np.array([v.camera_position.x, v.camera_position.y, v.camera_position.z,
                        v.forward.x, v.forward.y, v.forward.z, v.up.x, v.up.y, v.up.z,
                        v.vertical_fov] +
                       [c for vec in (v.min_coord, v.inv_dimensions, v.scaled_right, v.scaled_up,
                                      v.near_plane_top_left) for c in (vec.x, vec.y, vec.z)] +
                       [v.inv_width, v.inv_height, v.exposure, 0.0, 0.0], dtype=np.float32)
        return dict(spheres=arr(v.spheres, v.sphere_count, 4),
                    triangles=arr(v.triangles, v.triangle_count, 12),
                    material_indices=arr(v.material_indices, v.sphere_count + v.triangle_count, 0, np.uint16),
                    materials=arr(v.materials, v.material_count, 12),
                    bvh=arr(v.bvh, v.bvh_node_count, 8),
                    env=arr(v.environment_map, v.environment_map_width * v.environment_map_height, 3),
                    camera=cam)


def _vertices_np(vertices):
    """Validates refit vertices given as numpy: (n, 9) float32, contiguous; nothing is converted."""
    a = vertices
    if not isinstance(a, np.ndarray):
        raise ValueError("vertices must be a numpy array, not %s" % type(a).__name__)
    if a.dtype != np.float32:
        raise ValueError("vertices must be float32, not %s" % a.dtype)
    if a.ndim != 2 or a.shape[1] != 9:
        raise ValueError("vertices must have shape (n, 9), not %s" % (a.shape,))
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("vertices must be contiguous")
    return a


def default_opts(sort=True, device=0, pass_begin=0, pass_count=-1, pass_stride=1, counters=False,
                 tiles=None):
    """tiles = (tile_count, tile_index[, tile_rows]): render only that owner's row stripes."""
    o = RtOpts()
    lib().rt_default_opts(C.byref(o))
    o.sort, o.device, o.pass_begin, o.pass_count = int(sort), device, pass_begin, pass_count
    o.pass_stride, o.collect_counters = pass_stride, int(counters)
    if tiles is not None:
        o.tile_count, o.tile_index = tiles[0], tiles[1]
        o.tile_rows = tiles[2] if len(tiles) > 2 else 0
    return o


def tile_rows_of(height, tile_count, tile_index, tile_rows=8):
    """Image rows owned by tile_index: stripes of tile_rows rows dealt round-robin (rt_opts)."""
    rows = []
    for k in range(tile_index, -(-height // tile_rows), tile_count):
        rows.extend(range(k * tile_rows, min((k + 1) * tile_rows, height)))
    return rows


def render(scene, sort=True, device=0, pass_begin=0, pass_count=-1, pass_stride=1, counters=False,
           tiles=None, devices=None, shard_tiles=False, L=None):
    """rt_render: the drop-in for gpu_raytrace.  Returns (framebuffer W*H*3 float32, stats).
    devices = list of device ordinals: the in-library multi-GPU render (pass sharding + RCCL
    slice exchange and gather; rt_opts.device_count/device_ids), also at one device.
    L = the library to call (default lib(); tests: test_lib())."""
    L = L or lib()
    fb = np.zeros(scene.pixels * 3, np.float32)
    st = RtStats()
    o = default_opts(sort, device, pass_begin, pass_count, pass_stride, counters, tiles)
    ids = None
    if devices is not None:
        ids = (I32 * len(devices))(*[int(d) for d in devices])
        o.device_count = len(devices)
        o.device_ids = C.cast(ids, C.POINTER(I32))
        o.shard_tiles = int(shard_tiles)
    _check(L.rt_render(scene.ptr, C.byref(o), _ptr(fb), C.byref(st)), L)
    return fb, st.as_dict()


class MultiRenderer:
    """rt_multi: the persistent in-library multi-GPU renderer (one process, one RCCL communicator over
    `devices`, pass sharding with the slice exchange; the frame is gathered on devices[0])."""

    def __init__(self, scene, devices, sort=True, counters=False, L=None):
        self.L = L or lib()
        self.scene = scene
        o = default_opts(sort, int(devices[0]) if devices else 0, counters=counters)
        self._ids = (I32 * len(devices))(*[int(d) for d in devices])
        o.device_count = len(devices)
        o.device_ids = C.cast(self._ids, C.POINTER(I32))
        h = P()
        _check(self.L.rt_multi_create(scene.ptr, C.byref(o), C.byref(h)), self.L)
        self.h = h
        self.devices = len(devices)

    def run(self, pass_count=-1, host=False):
        """Renders passes 0..pass_count-1 of the frame over the devices; returns stats (and the frame
        when host=True: (fb, stats))."""
        st = RtStats()
        fb = np.zeros(self.scene.pixels * 3, np.float32) if host else None
        _check(self.L.rt_multi_run(self.h, int(pass_count), _ptr(fb) if host else None, C.byref(st)), self.L)
        return (fb, st.as_dict()) if host else st.as_dict()

    def framebuffer(self):
        fb = np.zeros(self.scene.pixels * 3, np.float32)
        _check(self.L.rt_multi_read_framebuffer(self.h, _ptr(fb)), self.L)
        return fb

    @property
    def ranks(self):
        return self.L.rt_multi_ranks(self.h)

    def set_event_timing(self, on):
        _check(self.L.rt_multi_set_event_timing(self.h, int(on)), self.L)

    def set_counters(self, on):
        _check(self.L.rt_multi_set_counters(self.h, int(on)), self.L)

    def close(self):
        if getattr(self, "h", None):
            self.L.rt_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


RCCL_ID_BYTES = 128   # RT_RCCL_ID_BYTES


def rccl_unique_id():
    """rt_rccl_unique_id: a new RCCL communicator id (bytes) for set_exchange_rccl."""
    buf = (C.c_uint8 * RCCL_ID_BYTES)()
    f = lib().rt_rccl_unique_id
    f.argtypes = [P]
    _check(f(buf))
    return bytes(buf)


def trace_rays(scene, rays, device=0, counters=False):
    """rt_trace_rays: closest hit of rays (n, 6) float32 {o.xyz, d.xyz}.  Returns (t, index, stats)."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = rays.shape[0]
    t = np.zeros(n, np.float32)
    idx = np.zeros(n, np.int32)
    st = RtStats()
    o = default_opts(True, device, counters=counters)
    _check(lib().rt_trace_rays(scene.ptr, C.byref(o), _ptr(rays), n, _ptr(t), _ptr(idx), C.byref(st)))
    return t, idx, st.as_dict()


def _is_tensor(x):
    """A torch.Tensor, told without importing torch (a numpy caller never pays for it)."""
    t = type(x)
    return t.__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr") and hasattr(x, "is_contiguous")


def _signed_distance(obj, points, direction):
    """signed_distance of a RayQuery or a Scene: closest_point's distance, negated where the count-only multi_hit
    along `direction` is odd."""
    d = np.asarray(direction, np.float32)
    if d.shape != (3,):
        raise ValueError("direction must have 3 components, not shape %s" % (d.shape,))
    dist = obj.closest_point(points, fields=("distance",))["distance"]
    if _is_tensor(points):
        import torch
        rays = torch.cat([points, torch.from_numpy(d).to(points.device).expand(points.shape[0], 3)], 1).contiguous()
        odd = (obj.multi_hit(rays, 1)[2] & 1).bool()
        return torch.where(odd, -dist, dist)
    rays = np.ascontiguousarray(np.hstack([_points_np(points), np.tile(d, (dist.shape[0], 1))]), np.float32)
    odd = (obj.multi_hit(rays, 1)[2] & 1).astype(bool)
    return np.where(odd, -dist, dist).astype(np.float32)


class RayQuery:
    """rt_query: resident ray queries (scene + BVH in HBM, scratch kept between calls).

    closest(rays) -> (t, index) and occluded(rays, tmax=None) -> mask take rays (n, 6) float32
    {o.xyz, d.xyz}, either as a numpy array (host path: rt_query_*_host, blocking, numpy results) or as a
    torch.Tensor on cuda:<device> (float32, shape (n, 6), contiguous; anything else raises ValueError,
    nothing is copied or converted silently).  For a tensor the results are torch tensors on that device
    (float32 t, int32 index, bool mask) and the work is enqueued on torch.cuda.current_stream(device)
    without any synchronisation: they are ready in stream order, like any torch op's.
    closest_hit(rays, fields=...) is closest with the hit record (uv, normal, position, material, front_face),
    and multi_hit(rays, k, tmax=None) -> (t, index, count) the k nearest hits in order with the crossing count,
    under the same rules; closest_point(points, max_dist=None) is the point query (nearest surface point, distance,
    index, uv), nearest_k(points, k, max_dist=None) the range query (every primitive within max_dist, the k nearest in
    order with their count) and signed_distance closest_point's composition with the crossing parity; update(vertices) moves the triangles under
    the frozen BVH topology.  closest_filtered and occluded_filtered are closest_hit and occluded over the surfaces a
    per-ray filter lets count (tmin, tmax, skip, mask against the primitive mask words of set_masks).
    hemisphere(points, normals, samples) counts, per surface point, the sample rays over the hemisphere above it that
    escape (made on the device, walked as occluded_filtered walks them), and ambient_occlusion is its openness in cosine
    mode.  overlap_box(boxes, k) is the volume query: every primitive whose surface meets an axis-aligned box,
    the k smallest indices, their count and an any flag."""

    def __init__(self, scene, device=0, counters=False, L=None):
        self.L = L or lib()
        self.scene = scene
        self.device = int(device)
        self.h = None
        f = self.L
        f.rt_query_create.argtypes = [P, P, C.POINTER(P)]
        f.rt_query_reserve.argtypes = [P, I32]
        f.rt_query_closest.argtypes = [P, P, I32, P, P, P]
        f.rt_query_occluded.argtypes = [P, P, P, I32, P, P]
        f.rt_query_closest_host.argtypes = [P, P, I32, P, P]
        f.rt_query_occluded_host.argtypes = [P, P, P, I32, P]
        f.rt_query_stats.argtypes = [P, P]
        f.rt_query_destroy.argtypes = [P]
        o = default_opts(True, self.device, counters=counters)
        h = P()
        _check(f.rt_query_create(scene.ptr, C.byref(o), C.byref(h)), f)
        self.h = h

    @classmethod
    def from_mesh(cls, *args, device=0, counters=False, **kwargs):
        """RayQuery(Scene.from_mesh(...), device, counters): resident queries on a mesh held in arrays.  The scene
        stays alive as .scene; its face_index maps answer indices back to the input faces."""
        return cls(Scene.from_mesh(*args, **kwargs), device, counters)

    @staticmethod
    def check_tensor(x, device, what="rays", shape_tail=(6,)):
        """Validates a torch tensor argument (float32, shape (n,) + shape_tail, contiguous, on
        cuda:<device>) with ValueError, before any library call; returns n."""
        import torch
        if x.dtype != torch.float32:
            raise ValueError("%s must be float32, not %s" % (what, x.dtype))
        if x.dim() != len(shape_tail) + 1 or tuple(x.shape[1:]) != tuple(shape_tail):
            raise ValueError("%s must have shape (n%s), not %s" % (what, "".join(", %d" % s for s in shape_tail),
                                                                  tuple(x.shape)))
        if not x.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        if x.device.type != "cuda" or x.device.index != int(device):
            raise ValueError("%s must be on cuda:%d, not %s" % (what, int(device), x.device))
        return int(x.shape[0])

    @staticmethod
    def _rays_np(rays):
        a = np.asarray(rays)
        if a.dtype != np.float32:
            raise ValueError("rays must be float32, not %s" % a.dtype)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError("rays must have shape (n, 6), not %s" % (a.shape,))
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("rays must be contiguous")
        return a

    def reserve(self, n):
        """Size the scratch for n rays now (later calls of up to n rays allocate nothing)."""
        _check(self.L.rt_query_reserve(self.h, int(n)), self.L)

    def closest(self, rays):
        """Closest hit: t (1e30 on a miss) and primitive index (-1 on a miss), as trace_rays."""
        if _is_tensor(rays):
            import torch
            n = self.check_tensor(rays, self.device)
            t = torch.empty(n, dtype=torch.float32, device=rays.device)
            idx = torch.empty(n, dtype=torch.int32, device=rays.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _check(self.L.rt_query_closest(self.h, P(rays.data_ptr()), n, P(t.data_ptr()), P(idx.data_ptr()),
                                           P(stream) if stream else None), self.L)
            return t, idx
        a = self._rays_np(rays)
        n = a.shape[0]
        t = np.zeros(n, np.float32)
        idx = np.zeros(n, np.int32)
        _check(self.L.rt_query_closest_host(self.h, _ptr(a), n, _ptr(t), _ptr(idx)), self.L)
        return t, idx

    def closest_hit(self, rays, fields=HIT_FIELDS):
        """rt_query_closest_hit: the closest hit with its hit record.  Returns a dict of the
        requested fields: t (n,) float32, index (n,) int32, uv (n, 2), normal (n, 3) (unflipped), position (n, 3)
        float32, material (n,) int32, front_face (n,) bool; a miss has index -1, material -1 and zeros.  Fields
        that are not requested are neither computed into memory nor allocated; fields=() only traverses and
        counts.  Tensors in, tensors out on torch.cuda.current_stream(device) without any synchronisation; a
        numpy array takes the _host path (blocking) and gives numpy.  An unknown field name raises ValueError."""
        names = _hit_fields(fields)
        f = self.L
        if _is_tensor(rays):
            import torch
            n = self.check_tensor(rays, self.device)
            dt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.bool}
            out = {k: torch.empty((n,) + HIT_SHAPES[k][0], dtype=dt[HIT_SHAPES[k][1]], device=rays.device) for k in names}
            ho = RtHitOut(**{k: v.data_ptr() for k, v in out.items()})
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_closest_hit.argtypes = [P, P, I32, P, P]
            _check(f.rt_query_closest_hit(self.h, P(rays.data_ptr()), n, C.byref(ho), P(stream) if stream else None), f)
            return out
        a = self._rays_np(rays)
        n = a.shape[0]
        out = {k: np.zeros((n,) + HIT_SHAPES[k][0], HIT_SHAPES[k][1]) for k in names}
        ho = RtHitOut(**{k: _ptr(v) for k, v in out.items()})
        f.rt_query_closest_hit_host.argtypes = [P, P, I32, P]
        _check(f.rt_query_closest_hit_host(self.h, _ptr(a), n, C.byref(ho)), f)
        if "front_face" in out:
            out["front_face"] = out["front_face"].view(np.bool_)
        return out

    def occluded(self, rays, tmax=None):
        """Any hit before tmax (per ray; None = 1e30, i.e. anything at all): a bool mask."""
        if _is_tensor(rays):
            import torch
            n = self.check_tensor(rays, self.device)
            if tmax is not None:
                if not _is_tensor(tmax):
                    raise ValueError("tmax must be a torch.Tensor when rays is one")
                if self.check_tensor(tmax, self.device, "tmax", ()) != n:
                    raise ValueError("tmax must have one entry per ray")
            mask = torch.empty(n, dtype=torch.bool, device=rays.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _check(self.L.rt_query_occluded(self.h, P(rays.data_ptr()), P(tmax.data_ptr()) if tmax is not None else None,
                                            n, P(mask.data_ptr()), P(stream) if stream else None), self.L)
            return mask
        a = self._rays_np(rays)
        n = a.shape[0]
        tm = None
        if tmax is not None:
            tm = np.asarray(tmax)
            if tm.dtype != np.float32 or tm.shape != (n,) or not tm.flags["C_CONTIGUOUS"]:
                raise ValueError("tmax must be a contiguous float32 array of shape (n,)")
        occ = np.zeros(n, np.uint8)
        _check(self.L.rt_query_occluded_host(self.h, _ptr(a), _ptr(tm) if tm is not None else None, n, _ptr(occ)),
               self.L)
        return occ.view(np.bool_)

    def multi_hit(self, rays, k, tmax=None):
        """rt_query_multi_hit: every hit before tmax (per ray; None = 1e30), the k nearest kept in order
        (DESIGN §14).  Returns (t (n, k) float32, index (n, k) int32, count (n,) int32): count is the number of
        surfaces the ray crosses, not capped by k; row entries past min(count, k) are (1e30, -1).  1 <= k <= 64.
        Tensors in, tensors out on torch.cuda.current_stream(device) without any synchronisation (tmax then a
        tensor too); a numpy array takes the _host path (blocking) and gives numpy."""
        k = _multi_hit_k(k)
        f = self.L
        if _is_tensor(rays):
            import torch
            n = self.check_tensor(rays, self.device)
            if tmax is not None:
                if not _is_tensor(tmax):
                    raise ValueError("tmax must be a torch.Tensor when rays is one")
                if self.check_tensor(tmax, self.device, "tmax", ()) != n:
                    raise ValueError("tmax must have one entry per ray")
            t = torch.empty((n, k), dtype=torch.float32, device=rays.device)
            idx = torch.empty((n, k), dtype=torch.int32, device=rays.device)
            cnt = torch.empty(n, dtype=torch.int32, device=rays.device)
            mo = RtMultiHitOut(t.data_ptr(), idx.data_ptr(), cnt.data_ptr())
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_multi_hit.argtypes = [P, P, P, I32, I32, P, P]
            _check(f.rt_query_multi_hit(self.h, P(rays.data_ptr()), P(tmax.data_ptr()) if tmax is not None else None, n, k,
                                        C.byref(mo), P(stream) if stream else None), f)
            return t, idx, cnt
        a = self._rays_np(rays)
        n = a.shape[0]
        tm = _tmax_np(tmax, n)
        t, idx, cnt = np.zeros((n, k), np.float32), np.zeros((n, k), np.int32), np.zeros(n, np.int32)
        mo = RtMultiHitOut(_ptr(t), _ptr(idx), _ptr(cnt))
        f.rt_query_multi_hit_host.argtypes = [P, P, P, I32, I32, P]
        _check(f.rt_query_multi_hit_host(self.h, _ptr(a), _ptr(tm) if tm is not None else None, n, k, C.byref(mo)), f)
        return t, idx, cnt

    def closest_point(self, points, max_dist=None, fields=CLOSEST_POINT_FIELDS):
        """rt_query_closest_point: for each point the nearest surface point within max_dist (per point, inclusive;
        None = unbounded) on the resident geometry.  Returns a dict of the requested fields: distance
        (n,) float32 (1e30 on a miss), index (n,) int32 (spheres first, then sphere_count + triangle; -1 on a miss),
        point (n, 3) and uv (n, 2) float32 (the point lies at p1 + u e1 + v e2 of the triangle; zeros on a miss and
        (0, 0) on a sphere).  Fields that are not requested are neither computed into memory nor allocated;
        fields=() only traverses and counts.  points (n, 3) float32, contiguous: a torch.Tensor on cuda:<device>
        (max_dist then a tensor too) gives tensors on torch.cuda.current_stream(device) without any synchronisation;
        a numpy array takes the _host path (blocking) and gives numpy.  Anything else raises ValueError."""
        names = _closest_point_fields(fields)
        f = self.L
        if _is_tensor(points):
            import torch
            n = self.check_tensor(points, self.device, "points", shape_tail=(3,))
            if max_dist is not None:
                if not _is_tensor(max_dist):
                    raise ValueError("max_dist must be a torch.Tensor when points is one")
                if self.check_tensor(max_dist, self.device, "max_dist", ()) != n:
                    raise ValueError("max_dist must have one entry per point")
            dt = {np.float32: torch.float32, np.int32: torch.int32}
            out = {k: torch.empty((n,) + CLOSEST_POINT_SHAPES[k][0], dtype=dt[CLOSEST_POINT_SHAPES[k][1]],
                                  device=points.device) for k in names}
            co = RtClosestPointOut(**{k: v.data_ptr() for k, v in out.items()})
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_closest_point.argtypes = [P, P, P, I32, P, P]
            _check(f.rt_query_closest_point(self.h, P(points.data_ptr()),
                                            P(max_dist.data_ptr()) if max_dist is not None else None, n, C.byref(co),
                                            P(stream) if stream else None), f)
            return out
        a = _points_np(points)
        n = a.shape[0]
        md = _max_dist_np(max_dist, n)
        out = {k: np.zeros((n,) + CLOSEST_POINT_SHAPES[k][0], CLOSEST_POINT_SHAPES[k][1]) for k in names}
        co = RtClosestPointOut(**{k: _ptr(v) for k, v in out.items()})
        f.rt_query_closest_point_host.argtypes = [P, P, P, I32, P]
        _check(f.rt_query_closest_point_host(self.h, _ptr(a), _ptr(md) if md is not None else None, n, C.byref(co)), f)
        return out

    def nearest_k(self, points, k, max_dist=None, fields=NEAREST_K_FIELDS):
        """rt_query_nearest_k: for each point every primitive within max_dist (per point, inclusive; None = unbounded)
        on the resident geometry, the k nearest kept in order.  Returns a dict of the requested fields:
        distance (n, k) float32, index (n, k) int32, point (n, k, 3) float32 and count (n,) int32 -- count is the number
        of primitives within max_dist, not capped by k; row entries past min(count, k) are (1e30, -1, zeros).
        1 <= k <= 64.  Fields that are not requested are neither written nor allocated; fields=() only traverses and
        counts.  points and max_dist as for closest_point: tensors in, tensors out on
        torch.cuda.current_stream(device) without any synchronisation; a numpy array takes the _host path (blocking)
        and gives numpy.  Anything else raises ValueError."""
        k, names = _nearest_k_args(k, fields)
        f = self.L
        if _is_tensor(points):
            import torch
            n = self.check_tensor(points, self.device, "points", shape_tail=(3,))
            if max_dist is not None:
                if not _is_tensor(max_dist):
                    raise ValueError("max_dist must be a torch.Tensor when points is one")
                if self.check_tensor(max_dist, self.device, "max_dist", ()) != n:
                    raise ValueError("max_dist must have one entry per point")
            dt = {np.float32: torch.float32, np.int32: torch.int32}
            out = {x: torch.empty(_nearest_k_shape(x, n, k), dtype=dt[NEAREST_K_DTYPES[x]], device=points.device)
                   for x in names}
            no = RtNearestKOut(**{x: v.data_ptr() for x, v in out.items()})
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_nearest_k.argtypes = [P, P, P, I32, I32, P, P]
            _check(f.rt_query_nearest_k(self.h, P(points.data_ptr()),
                                        P(max_dist.data_ptr()) if max_dist is not None else None, n, k, C.byref(no),
                                        P(stream) if stream else None), f)
            return out
        a = _points_np(points)
        n = a.shape[0]
        md = _max_dist_np(max_dist, n)
        out = {x: np.zeros(_nearest_k_shape(x, n, k), NEAREST_K_DTYPES[x]) for x in names}
        no = RtNearestKOut(**{x: _ptr(v) for x, v in out.items()})
        f.rt_query_nearest_k_host.argtypes = [P, P, P, I32, I32, P]
        _check(f.rt_query_nearest_k_host(self.h, _ptr(a), _ptr(md) if md is not None else None, n, k, C.byref(no)), f)
        return out

    def overlap_box(self, boxes, k, fields=("index", "count")):
        """rt_query_overlap_box: for each axis-aligned box {lo.xyz, hi.xyz} every primitive whose surface meets it on the
        resident geometry.  Returns a dict of the requested fields: index (n, k) int32 -- the min(count, k)
        smallest member indices ascending (spheres first, then sphere_count + triangle), then -1 --, count (n,) int32,
        not capped by k, and any (n,) uint8.  1 <= k <= 64.  A box with a non-finite number or lo > hi on an axis meets
        nothing.  Fields that are not requested are neither written nor allocated; fields=("any",) stops each box's walk
        at its first member, fields=() only traverses and counts.  boxes (n, 6) float32, contiguous: a torch.Tensor on
        cuda:<device> gives tensors on torch.cuda.current_stream(device) without any synchronisation; a numpy array
        takes the _host path (blocking) and gives numpy.  Anything else raises ValueError."""
        k, names = _overlap_args(k, fields)
        f = self.L
        if _is_tensor(boxes):
            import torch
            n = self.check_tensor(boxes, self.device, "boxes", shape_tail=(6,))
            dt = {np.int32: torch.int32, np.uint8: torch.uint8}
            out = {x: torch.empty(_overlap_shape(x, n, k), dtype=dt[OVERLAP_DTYPES[x]], device=boxes.device) for x in names}
            oo = RtOverlapOut(**{x: v.data_ptr() for x, v in out.items()})
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_overlap_box.argtypes = [P, P, I32, I32, P, P]
            _check(f.rt_query_overlap_box(self.h, P(boxes.data_ptr()), n, k, C.byref(oo), P(stream) if stream else None), f)
            return out
        a = _boxes_np(boxes)
        n = a.shape[0]
        out = {x: np.zeros(_overlap_shape(x, n, k), OVERLAP_DTYPES[x]) for x in names}
        oo = RtOverlapOut(**{x: _ptr(v) for x, v in out.items()})
        f.rt_query_overlap_box_host.argtypes = [P, P, I32, I32, P]
        _check(f.rt_query_overlap_box_host(self.h, _ptr(a), n, k, C.byref(oo)), f)
        return out

    @staticmethod
    def _check_member_tensor(x, device, what, dtypes):
        """check_tensor's rules for a per-ray filter member or the mask words: a 1-D contiguous tensor on
        cuda:<device> of one of the torch dtypes named in `dtypes`; returns its length."""
        import torch
        if not _is_tensor(x):
            raise ValueError("%s must be a torch.Tensor when rays is one" % what)
        allowed = [getattr(torch, d) for d in dtypes if hasattr(torch, d)]
        if x.dtype not in allowed:
            raise ValueError("%s must be %s, not %s" % (what, " or ".join(dtypes), x.dtype))
        if x.dim() != 1:
            raise ValueError("%s must have shape (n), not %s" % (what, tuple(x.shape)))
        if not x.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        if x.device.type != "cuda" or x.device.index != int(device):
            raise ValueError("%s must be on cuda:%d, not %s" % (what, int(device), x.device))
        return int(x.shape[0])

    _FILTER_TORCH = {"tmin": ("float32",), "tmax": ("float32",), "skip": ("int32",), "mask": ("uint32", "int32")}

    def _filter_tensors(self, n, **members):
        """The filter members given as tensors (None = not given), validated; an int32 mask is read as its bits."""
        ptrs = {}
        for name, dtypes in self._FILTER_TORCH.items():
            v = members.get(name)
            if v is None:
                continue
            if self._check_member_tensor(v, self.device, name, dtypes) != n:
                raise ValueError("%s must have one entry per ray" % name)
            ptrs[name] = v.data_ptr()
        return RtRayFilter(**ptrs)

    def set_masks(self, masks):
        """rt_query_set_masks: the primitive mask words, one uint32 per primitive in the public numbering (spheres
        first), or None to drop them (every primitive's word is then 0xFFFFFFFF).  A numpy uint32 array goes through
        the _host call (blocking); a torch.Tensor on cuda:<device> (uint32, or int32 read as its bits) is copied on
        torch.cuda.current_stream(device) without any synchronisation: calls enqueued earlier see the old masks, later
        ones the new.  The masks survive update().  Anything else raises ValueError."""
        f = self.L
        count = self.scene.view.sphere_count + self.scene.view.triangle_count if self.scene is not None else None
        if masks is None:
            f.rt_query_set_masks_host.argtypes = [P, P, I32]
            _check(f.rt_query_set_masks_host(self.h, None, count), f)
            return
        if _is_tensor(masks):
            import torch
            n = self._check_member_tensor(masks, self.device, "masks", ("uint32", "int32"))
            if count is not None and n != count:
                raise ValueError("masks must have sphere_count + triangle_count = %d words, not %d" % (count, n))
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_set_masks.argtypes = [P, P, I32, P]
            _check(f.rt_query_set_masks(self.h, P(masks.data_ptr()), n, P(stream) if stream else None), f)
            return
        a = np.asarray(masks)
        a = _masks_np(a, a.shape[0] if count is None and a.ndim == 1 else count)
        f.rt_query_set_masks_host.argtypes = [P, P, I32]
        _check(f.rt_query_set_masks_host(self.h, _ptr(a), a.shape[0]), f)

    def closest_filtered(self, rays, tmin=None, tmax=None, skip=None, mask=None, fields=("t", "index")):
        """rt_query_closest_filtered: the closest hit among the surfaces that count for each ray: hits in
        [max(tmin, 0.005), min(tmax, 1e30)), not on primitive skip, on a primitive whose mask word (set_masks) shares a
        bit with the ray's `mask`.  Every member is None or one entry per ray (tmin, tmax float32, skip int32, mask
        uint32).  Returns a dict of the requested hit-record fields as closest_hit does (a miss has t 1e30, index -1);
        fields=() only traverses and counts.  The walk visits the near child first and is part of the call's
        definition; with no filter it need not return closest()'s index where two surfaces tie in t.  Tensors in
        (the members then tensors too), tensors out on torch.cuda.current_stream(device) without any synchronisation; a
        numpy array takes the _host path (blocking) and gives numpy.  Anything malformed raises ValueError."""
        names = _hit_fields(fields)
        f = self.L
        if _is_tensor(rays):
            import torch
            n = self.check_tensor(rays, self.device)
            rf = self._filter_tensors(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
            dt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.bool}
            out = {k: torch.empty((n,) + HIT_SHAPES[k][0], dtype=dt[HIT_SHAPES[k][1]], device=rays.device) for k in names}
            ho = RtHitOut(**{k: v.data_ptr() for k, v in out.items()})
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_closest_filtered.argtypes = [P, P, P, I32, P, P]
            _check(f.rt_query_closest_filtered(self.h, P(rays.data_ptr()), C.byref(rf), n, C.byref(ho),
                                               P(stream) if stream else None), f)
            return out
        a = self._rays_np(rays)
        n = a.shape[0]
        rf, keep = _filter_np(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        out = {k: np.zeros((n,) + HIT_SHAPES[k][0], HIT_SHAPES[k][1]) for k in names}
        ho = RtHitOut(**{k: _ptr(v) for k, v in out.items()})
        f.rt_query_closest_filtered_host.argtypes = [P, P, P, I32, P]
        _check(f.rt_query_closest_filtered_host(self.h, _ptr(a), C.byref(rf), n, C.byref(ho)), f)
        if "front_face" in out:
            out["front_face"] = out["front_face"].view(np.bool_)
        return out

    def occluded_filtered(self, rays, tmin=None, tmax=None, skip=None, mask=None):
        """rt_query_occluded_filtered: whether any surface that counts for the ray (closest_filtered's filter) lies in
        its interval: a bool mask, equal to closest_filtered's index >= 0 under the same filter.  Arguments and paths
        as closest_filtered's."""
        f = self.L
        if _is_tensor(rays):
            import torch
            n = self.check_tensor(rays, self.device)
            rf = self._filter_tensors(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
            occ = torch.empty(n, dtype=torch.bool, device=rays.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_occluded_filtered.argtypes = [P, P, P, I32, P, P]
            _check(f.rt_query_occluded_filtered(self.h, P(rays.data_ptr()), C.byref(rf), n, P(occ.data_ptr()),
                                                P(stream) if stream else None), f)
            return occ
        a = self._rays_np(rays)
        n = a.shape[0]
        rf, keep = _filter_np(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        occ = np.zeros(n, np.uint8)
        f.rt_query_occluded_filtered_host.argtypes = [P, P, P, I32, P]
        _check(f.rt_query_occluded_filtered_host(self.h, _ptr(a), C.byref(rf), n, _ptr(occ)), f)
        return occ.view(np.bool_)

    def hemisphere(self, points, normals, samples, mode="cosine", seed=0, point_offset=0, tmin=None, tmax=None, skip=None,
                   mask=None, fields=HEMISPHERE_FIELDS):
        """rt_query_hemisphere: how open the hemisphere above each surface point is.  points and normals
        (n, 3) float32; `samples` rays per point (1..4096) are made on the device from (seed, point_offset + i, s) --
        mode "cosine" (cosine-weighted about the normal) or "uniform" -- and walked as occluded_filtered walks them
        under the point's filter row: tmin, tmax (the AO radius), skip (the point's own primitive), mask against the
        set_masks words, each None or one entry per point.  Returns a dict of the requested fields: open_count (n,)
        int32, the rays that escaped, and openness (n,) float32 = open_count / samples.  The counts are exactly
        reproducible; a batch split into parts called with point_offset = the part's first row gives the whole
        batch's rows; hemisphere_rays() returns the rays a call stands for.  Tensors in (the members then tensors too),
        tensors out on torch.cuda.current_stream(device) without any synchronisation; numpy takes the _host path
        (blocking) and gives numpy.  Anything malformed raises ValueError before the library is called."""
        names = _hemisphere_fields(fields)
        f = self.L
        if _is_tensor(points):
            import torch
            if not _is_tensor(normals):
                raise ValueError("normals must be a torch.Tensor when points is one")
            n = self.check_tensor(points, self.device, "points", (3,))
            if self.check_tensor(normals, self.device, "normals", (3,)) != n:
                raise ValueError("normals must have one row per point")
            hp = _hemisphere_params(n, samples, mode, seed, point_offset)
            rf = self._filter_tensors(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
            frames = torch.cat([points, normals], 1)
            dt = {np.float32: torch.float32, np.int32: torch.int32}
            out = {k: torch.empty(n, dtype=dt[HEMISPHERE_DTYPES[k]], device=points.device) for k in names}
            ho = RtHemisphereOut(**{k: v.data_ptr() for k, v in out.items()})
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_hemisphere.argtypes = [P, P, P, I32, P, P, P]
            _check(f.rt_query_hemisphere(self.h, P(frames.data_ptr()), C.byref(rf), n, C.byref(hp), C.byref(ho),
                                         P(stream) if stream else None), f)
            return out
        if _is_tensor(normals):
            raise ValueError("normals must be a numpy array when points is one")
        fr = _frames_np(points, normals)
        n = fr.shape[0]
        hp = _hemisphere_params(n, samples, mode, seed, point_offset)
        rf, keep = _filter_np(n, tmin=tmin, tmax=tmax, skip=skip, mask=mask)
        out = {k: np.zeros(n, HEMISPHERE_DTYPES[k]) for k in names}
        ho = RtHemisphereOut(**{k: _ptr(v) for k, v in out.items()})
        f.rt_query_hemisphere_host.argtypes = [P, P, P, I32, P, P]
        _check(f.rt_query_hemisphere_host(self.h, _ptr(fr), C.byref(rf), n, C.byref(hp), C.byref(ho)), f)
        return out

    def ambient_occlusion(self, points, normals, samples, radius=None, skip=None, seed=0):
        """hemisphere's openness in cosine mode: 1 = nothing within `radius` (None or one float32 per point; None =
        unbounded) above the point, 0 = fully enclosed.  skip: each point's own primitive, or None."""
        return self.hemisphere(points, normals, samples, "cosine", seed, 0, tmax=radius, skip=skip, fields=("openness",))["openness"]

    def signed_distance(self, points, direction=(0.5773503, 0.5773503, 0.5773503)):
        """closest_point's distance, negated where the point lies inside a closed mesh: a point is taken to be inside
        where the ray from it along `direction` (unit length) crosses an odd number of surfaces (the count-only
        multi_hit).  A composition of the two queries, Python only.  It is a parity test: a ray that grazes an
        edge or a vertex of the mesh, or runs inside a face's plane, can count a crossing twice or not at all and
        flip the sign, and an open mesh has no inside; hits nearer than 0.005 along the ray are not counted, as
        everywhere.  Misses of closest_point (non-finite points) keep 1e30.  points as for closest_point; returns a
        tensor or an array like it."""
        return _signed_distance(self, points, direction)

    def update(self, vertices):
        """rt_query_update_triangles: new vertices (n, 9) float32 {a.xyz, b.xyz, c.xyz} in the scene's
        triangle order, under the frozen BVH topology (a refit of the resident records).  A numpy array
        goes through the _host call (staged, blocking); a torch.Tensor on cuda:<device> is read in place
        and the work is enqueued on torch.cuda.current_stream(device) without any synchronisation.  Queries
        enqueued afterwards, on any stream, see the new geometry.  Anything else raises ValueError."""
        f = self.L
        if _is_tensor(vertices):
            import torch
            n = self.check_tensor(vertices, self.device, "vertices", shape_tail=(9,))
            stream = torch.cuda.current_stream(self.device).cuda_stream
            f.rt_query_update_triangles.argtypes = [P, P, I32, P]
            _check(f.rt_query_update_triangles(self.h, P(vertices.data_ptr()), n, P(stream) if stream else None), f)
            return
        a = _vertices_np(vertices)
        f.rt_query_update_triangles_host.argtypes = [P, P, I32]
        _check(f.rt_query_update_triangles_host(self.h, _ptr(a), a.shape[0]), f)

    def geometry(self):
        """rt_query_read_geometry: waits, then returns the device's current (triangles (n, 12), bvh (m, 8))
        as float32 arrays laid out like Scene.arrays()' (the bvh's last two columns are the int32 children)."""
        v = self.scene.view
        tri = np.zeros((v.triangle_count, 12), np.float32)
        bvh = np.zeros((v.bvh_node_count, 8), np.float32)
        f = self.L.rt_query_read_geometry
        f.argtypes = [P, P, P]
        _check(f(self.h, _ptr(tri), _ptr(bvh)), self.L)
        return tri, bvh

    def stats(self):
        """rt_query_stats: waits for the last call and returns its counters."""
        st = RtStats()
        _check(self.L.rt_query_stats(self.h, C.byref(st)), self.L)
        return st.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self.L.rt_query_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Renderer:
    """Persistent renderer (scene + ray buffers resident in HBM)."""

    def __init__(self, scene, sort=True, device=0, counters=False, tiles=None, L=None):
        """L = the library to call (default lib(); tests: test_lib())."""
        self.L = L or lib()
        self.scene = scene
        o = default_opts(sort, device, counters=counters, tiles=tiles)
        h = P()
        self._check(self.L.rt_renderer_create(scene.ptr, C.byref(o), C.byref(h)))
        self.h = h

    def _check(self, rc):
        _check(rc, self.L)

    def run(self, pass_begin=0, count=1, stride=1, d_pass_sums=None):
        st = RtStats()
        self._check(self.L.rt_renderer_run(self.h, pass_begin, count, stride,
                                     P(d_pass_sums) if d_pass_sums else None, C.byref(st)))
        return st.as_dict()

    def run_async(self, pass_begin=0, count=1, stride=1, d_pass_sums=None):
        """rt_renderer_run_async: enqueue the passes and return; then wait_pass / finish."""
        f = self.L.rt_renderer_run_async
        f.argtypes = [P, I32, I32, I32, P]
        self._check(f(self.h, pass_begin, count, stride, P(d_pass_sums) if d_pass_sums else None))

    def wait_pass(self, k, hip_stream):
        """The HIP stream `hip_stream` (a raw handle, e.g. torch.cuda.current_stream().cuda_stream)
        waits until pass k of the async run has written its sums."""
        f = self.L.rt_renderer_wait_pass
        f.argtypes = [P, I32, P]
        self._check(f(self.h, int(k), P(hip_stream) if hip_stream else None))

    def finish(self):
        st = RtStats()
        f = self.L.rt_renderer_finish
        f.argtypes = [P, P]
        self._check(f(self.h, C.byref(st)))
        return st.as_dict()

    def run_host(self, pass_begin=0, count=1, stride=1):
        """Renders passes and returns their per-pass sums (count, W*H*3) in host memory."""
        out = np.zeros((count, self.scene.pixels * 3), np.float32)
        st = RtStats()
        self._check(self.L.rt_renderer_run_host(self.h, pass_begin, count, stride, _ptr(out), C.byref(st)))
        return out, st.as_dict()

    def set_exchange(self, exchange=None, c_fn=None, user=None):
        """Pixel tiles with sort on (rt_renderer_set_exchange).  Either
        exchange(arr): sums the uint8 numpy array over all tile owners in place (host buffer,
        on_device = 0), or c_fn/user: a native rt_exchange_fn (a ctypes function pointer, e.g. from
        a loaded library) called with the device pointer and the pass's HIP stream (on_device = 1),
        which must enqueue its in-place sum on that stream."""
        f = self.L.rt_renderer_set_exchange
        if c_fn is not None:
            f.argtypes = [P, P, P, I32]
            self._exchange = (c_fn, user)   # kept alive as long as the renderer
            self._check(f(self.h, C.cast(c_fn, P), P(user) if user else None, 1))
            return

        def cb(user, p, n, stream):
            try:
                exchange(np.ctypeslib.as_array(p, shape=(int(n),)))
                return 0
            except Exception:           # reported by the renderer as a failed exchange
                return -1
        self._exchange = EXCHANGE(cb)  # kept alive as long as the renderer
        f.argtypes = [P, EXCHANGE, P, I32]
        self._check(f(self.h, self._exchange, None, 0))

    def set_exchange_rccl(self, unique_id, nranks, rank):
        """The exchange over an RCCL communicator the renderer joins (one process per GPU):
        rt_renderer_set_exchange_rccl.  unique_id: the RT_RCCL_ID_BYTES bytes rank 0 got from
        rccl_unique_id(), the same on every rank.  Blocks until every rank has joined."""
        f = self.L.rt_renderer_set_exchange_rccl
        f.argtypes = [P, P, I32, I32]
        buf = (C.c_uint8 * RCCL_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(f(self.h, buf, int(nranks), int(rank)))

    def set_counters(self, on):
        self._check(self.L.rt_renderer_set_counters(self.h, int(on)))

    def set_accumulate(self, on):
        """Framebuffer accumulation (rt_renderer_set_accumulate; default on).  Off: runs need d_pass_sums
        and only write them (the multi-GPU drivers add the pass slices themselves)."""
        f = self.L.rt_renderer_set_accumulate
        f.argtypes = [P, I32]
        self._check(f(self.h, int(on)))

    def launch_profile(self, cap=256):
        """Per trace launch of the last event-timed run's first pass: [(span ms, live rays), ...]
        (rt_renderer_launch_profile)."""
        f = self.L.rt_renderer_launch_profile
        f.argtypes = [P, I32, P, P]
        ms = np.zeros(cap, np.float64)
        live = np.zeros(cap, np.uint32)
        n = f(self.h, cap, _ptr(ms), _ptr(live))
        if n < 0:
            self._check(n)
        return [(float(ms[b]), int(live[b])) for b in range(n)]

    def set_event_timing(self, on):
        """Per-bounce HIP events for process_ms / sort_ms (default on; off is ~2 % faster)."""
        f = self.L.rt_renderer_set_event_timing
        f.argtypes = [P, I32]
        self._check(f(self.h, int(on)))

    def framebuffer(self):
        fb = np.zeros(self.scene.pixels * 3, np.float32)
        self._check(self.L.rt_renderer_read_framebuffer(self.h, _ptr(fb)))
        return fb

    def copy_framebuffer(self, d_out):
        """Device framebuffer -> device pointer d_out (W*H*3 float32 on the renderer's device)."""
        f = self.L.rt_renderer_copy_framebuffer
        f.argtypes = [P, P]
        self._check(f(self.h, P(d_out)))

    def clear(self):
        self._check(self.L.rt_renderer_clear(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.rt_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def bloom(fb, width, height, threshold, radius=5, device=0):
    out = np.array(fb, dtype=np.float32, copy=True)
    _check(lib().rt_bloom(_ptr(out), width, height, threshold, radius, device))
    return out


def bloom_device(ptr, width, height, threshold, radius=5, device=0):
    _check(lib().rt_bloom_device(P(ptr), width, height, threshold, radius, device))


def tonemap(fb, width, height, exposure, ray_count):
    out = np.zeros(width * height * 3, np.uint8)
    src = np.ascontiguousarray(fb, dtype=np.float32)
    lib().rt_tonemap(_ptr(src), width, height, exposure, ray_count, _ptr(out))
    return out


def write_png(path, rgb, width, height):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    _check(lib().rt_write_png(path.encode(), _ptr(rgb), width, height))


def cpu_render(scene, threads=0):
    """The reference's `cpu` path (rt_cpu_render). Returns (fb, seconds)."""
    fb = np.zeros(scene.pixels * 3, np.float32)
    secs = C.c_double(0)
    rc = lib().rt_cpu_render(scene.ptr, _ptr(fb), threads, C.byref(secs))
    if rc < 0:
        raise RtError(lib().rt_last_error().decode())
    return fb, secs.value
