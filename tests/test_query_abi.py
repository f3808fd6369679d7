"""The rt_query_* boundary (include/rt_abi.h) without a GPU: the symbols are declared and exported (their
presence is the feature probe; the ABI version stays 7), bad arguments are refused with a message before any
HIP call, and rtamd.RayQuery refuses tensors it would have to copy or convert."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import rtamd as R

QUERY_FUNCTIONS = ("rt_query_create", "rt_query_reserve", "rt_query_closest", "rt_query_occluded",
                   "rt_query_closest_host", "rt_query_occluded_host", "rt_query_stats", "rt_query_destroy")


def test_header_declares_the_query_functions():
    text = re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))
    assert set(QUERY_FUNCTIONS) <= names
    assert "typedef struct rt_query rt_query;" in text
    assert int(re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text).group(1)) == 7


@pytest.mark.parametrize("path", [R.LIB_PATH, R.TEST_LIB_PATH])
def test_libraries_export_the_query_functions(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines())
    assert set(QUERY_FUNCTIONS) <= exported


def test_abi_version_and_struct_sizes_unchanged():
    assert R.lib().rt_abi_version() == 7 and R.test_lib().rt_abi_version() == 7
    assert C.sizeof(R.RtOpts) == 56
    assert C.sizeof(R.RtStats) == 11 * 8 + 8 + 5 * 8 + 8 + 8


def _invalid(lib, rc, *words):
    assert rc == -1                                         # RT_E_INVALID
    msg = lib.rt_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_bad_arguments_are_refused_with_a_message():
    lib = R.lib()
    P, I32 = R.P, R.I32
    lib.rt_query_create.argtypes = [P, P, C.POINTER(P)]
    lib.rt_query_reserve.argtypes = [P, I32]
    lib.rt_query_closest.argtypes = [P, P, I32, P, P, P]
    lib.rt_query_occluded.argtypes = [P, P, P, I32, P, P]
    lib.rt_query_closest_host.argtypes = [P, P, I32, P, P]
    lib.rt_query_occluded_host.argtypes = [P, P, P, I32, P]
    lib.rt_query_stats.argtypes = [P, P]
    buf = np.zeros(64, np.float32)
    b = R._ptr(buf)
    # null object
    _invalid(lib, lib.rt_query_reserve(None, 4), "rt_query_reserve", "null")
    _invalid(lib, lib.rt_query_closest(None, b, 1, b, b, None), "rt_query_closest", "null")
    _invalid(lib, lib.rt_query_occluded(None, b, None, 1, b, None), "rt_query_occluded", "null")
    _invalid(lib, lib.rt_query_closest_host(None, b, 1, b, b), "rt_query_closest_host", "null")
    _invalid(lib, lib.rt_query_occluded_host(None, b, None, 1, b), "rt_query_occluded_host", "null")
    _invalid(lib, lib.rt_query_stats(None, None), "rt_query_stats", "null")
    _invalid(lib, lib.rt_query_create(None, None, None), "null")
    h = P()
    _invalid(lib, lib.rt_query_create(None, None, C.byref(h)), "null scene")
    assert not h.value
    lib.rt_query_destroy(None)                              # like free(NULL)
    # The count and the pointers are checked before the object is used at all (and before any HIP call), so
    # these calls never read `obj`: a block of zeros stands in for an object no GPU-less box can create.
    zeros = np.zeros(1 << 16, np.uint8)
    obj = R._ptr(zeros)
    _invalid(lib, lib.rt_query_reserve(obj, -1), "negative")
    _invalid(lib, lib.rt_query_closest(obj, b, -1, b, b, None), "negative")
    _invalid(lib, lib.rt_query_occluded(obj, b, None, -5, b, None), "negative")
    _invalid(lib, lib.rt_query_closest_host(obj, b, -1, b, b), "negative")
    _invalid(lib, lib.rt_query_occluded_host(obj, b, None, -1, b), "negative")
    for args in ((None, 1, b, b, None), (b, 1, None, b, None), (b, 1, b, None, None)):
        _invalid(lib, lib.rt_query_closest(obj, *args), "rt_query_closest", "null pointer")
    for args in ((None, None, 1, b, None), (b, None, 1, None, None)):
        _invalid(lib, lib.rt_query_occluded(obj, *args), "rt_query_occluded", "null pointer")
    for args in ((None, 1, b, b), (b, 1, None, b), (b, 1, b, None)):
        _invalid(lib, lib.rt_query_closest_host(obj, *args), "rt_query_closest_host", "null pointer")
    for args in ((None, None, 1, b), (b, None, 1, None)):
        _invalid(lib, lib.rt_query_occluded_host(obj, *args), "rt_query_occluded_host", "null pointer")
    # n == 0: RT_OK, no pointer touched
    assert lib.rt_query_closest(obj, None, 0, None, None, None) == 0
    assert lib.rt_query_occluded(obj, None, None, 0, None, None) == 0
    assert lib.rt_query_closest_host(obj, None, 0, None, None) == 0
    assert lib.rt_query_occluded_host(obj, None, None, 0, None) == 0


def test_create_without_a_device_is_nodevice():
    if R.device_count() != 0:
        return                                              # with a device: tests/test_gpu_query.py
    scene = R.Scene("%s/cornell.scene" % R.ASSETS, image=(16, 16, 1, 1))
    h = R.P()
    lib = R.lib()
    lib.rt_query_create.argtypes = [R.P, R.P, C.POINTER(R.P)]
    assert lib.rt_query_create(scene.ptr, None, C.byref(h)) == -4      # RT_E_NODEVICE
    assert b"device" in lib.rt_last_error() and not h.value
    with pytest.raises(R.RtError):
        R.RayQuery(scene)


def _unbound_query():
    """A RayQuery with no library and no object behind it: validation that reached the library would fail
    with AttributeError/TypeError instead of ValueError."""
    q = R.RayQuery.__new__(R.RayQuery)
    q.L, q.h, q.device, q.scene = None, None, 0, None
    return q


def test_rayquery_rejects_tensors_it_would_have_to_convert():
    import torch
    q = _unbound_query()
    good_shape = torch.zeros((10, 6), dtype=torch.float32)
    cases = {
        "float32": torch.zeros((10, 6), dtype=torch.float64),
        "shape": torch.zeros((10, 5), dtype=torch.float32),
        "shape ": torch.zeros(60, dtype=torch.float32),
        "contiguous": torch.zeros((10, 12), dtype=torch.float32)[:, ::2],
        "cuda:0": good_shape,                               # a CPU tensor: wrong device
    }
    for word, x in cases.items():
        for call in (q.closest, q.occluded, lambda r: R.RayQuery.check_tensor(r, 0)):
            with pytest.raises(ValueError, match=word.strip()):
                call(x)
    assert cases["contiguous"].shape == (10, 6) and not cases["contiguous"].is_contiguous()
    # numpy arrays: the same rules, nothing converted silently
    for x in (np.zeros((10, 6), np.float64), np.zeros((10, 5), np.float32), np.zeros((10, 12), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            q.closest(x)
        with pytest.raises(ValueError):
            q.occluded(x)
    with pytest.raises(ValueError, match="tmax"):
        q.occluded(np.zeros((10, 6), np.float32), tmax=np.zeros(9, np.float32))


def test_numpy_path_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import numpy as np, rtamd; "
            "q = rtamd.RayQuery.__new__(rtamd.RayQuery); q.L = q.h = None; q.device = 0\n"
            "try:\n    q.closest(np.zeros((4, 5), np.float32))\nexcept ValueError:\n    pass\n"
            "print('torch' in sys.modules)") % R.PKG_DIR
    out = subprocess.run([__import__("sys").executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["False"]
