"""CPU-only: the ABI of erasing from the map.  kf_brick_store_erase_box and kf_brick_store_erase_weak are exported, bound, declared with the argument
counts of include/hybkf.h and refuse a NULL context without a device; the host shim's names and the Python methods exist and answer -1 without an
application; the slab shim always answers -1.  hkf_erase_map_box_voxels (no application, no device) states the centre rule."""
import ctypes as C
import os
import re

import numpy as np

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1001


def declared_args(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_header_and_binding():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name, n in (("kf_brick_store_erase_box", 6), ("kf_brick_store_erase_weak", 3)):
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        args = declared_args(header, name)
        assert len(args) == n and args[0] == "kf_ctx* ctx", (name, args)
        assert len(getattr(lib, name).argtypes) == n, name
    assert declared_args(header, "kf_brick_store_erase_box")[1:] == ["const int32_t lo_vox[3]", "const int32_t hi_vox[3]", "int mode", "uint32_t* bricks_removed",
                                                                     "uint64_t* voxels_cleared"]
    assert declared_args(header, "kf_brick_store_erase_weak")[1:] == ["float min_weight", "uint32_t* bricks_removed"]
    assert re.search(r"^#define KF_ERASE_INSIDE 0$", header, re.M) and re.search(r"^#define KF_ERASE_OUTSIDE 1$", header, re.M)
    assert (K.ERASE_INSIDE, K.ERASE_OUTSIDE) == (0, 1)
    assert hasattr(K.Context, "brick_store_erase_box") and hasattr(K.Context, "brick_store_erase_weak")
    for name in ("erase_map_box", "erase_map_weak"):
        assert hasattr(H.App, name) and hasattr(H.SlabsApp, name), name


def test_null_context_is_refused_without_a_device():
    lib = K.load()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    removed, cleared = C.c_uint32(7), C.c_uint64(7)
    assert lib.kf_brick_store_erase_box(None, lo, hi, 0, C.byref(removed), C.byref(cleared)) == ARG
    assert lib.kf_brick_store_erase_box(None, lo, hi, 1, None, None) == ARG
    assert lib.kf_brick_store_erase_box(None, None, None, 2, None, None) == ARG
    assert lib.kf_brick_store_erase_weak(None, 1.0, C.byref(removed)) == ARG
    assert lib.kf_brick_store_erase_weak(None, float("nan"), None) == ARG
    assert (removed.value, cleared.value) == (7, 7)                # refused: nothing written


def test_shims_without_an_application():
    h = H.load()
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    for name in ("hkf_app_erase_map_box", "hkf_app_erase_map_weak", "hkf_erase_map_box_voxels"):
        assert hasattr(h, name), name
    assert h.hkf_app_erase_map_box(lo, hi, 0, None) == -1 and h.hkf_app_erase_map_weak(C.c_float(2.0), None) == -1
    s = H.load_slabs()
    assert s.hkf_slabs_erase_map_box(lo, hi, 0, None) == -1 and s.hkf_slabs_erase_map_weak(C.c_float(2.0), None) == -1


def test_metres_to_voxels_is_the_centre_rule():
    """cell 1 / 32: voxel g has its centre at (g + 1/2) / 32; a voxel is in the box iff lo <= centre < hi"""
    h = H.load()
    cell = np.float32(1.0 / 32)
    lo_m = np.array([-0.25, 2.5 / 32, -1.0], np.float32)          # on a voxel border; exactly on the centre of voxel 2; on a border
    hi_m = np.array([0.26, 2.5 / 32, np.inf], np.float32)
    lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    assert h.hkf_erase_map_box_voxels(lo_m.ctypes.data_as(C.c_void_p), hi_m.ctypes.data_as(C.c_void_p), C.c_float(cell), lo, hi) == 0
    g = np.arange(-100, 100)
    centre = (g + 0.5) * float(cell)
    for k in range(2):
        inside = g[(centre >= float(lo_m[k])) & (centre < float(hi_m[k]))]
        if len(inside):
            assert (lo[k], hi[k]) == (inside[0], inside[-1] + 1), k
        else:
            assert lo[k] >= hi[k], k
    assert (lo[0], hi[0]) == (-8, 8) and lo[1] == hi[1] == 2       # 0.26 * 32 = 8.32: voxel 8's centre, 8.5, is outside
    assert (lo[2], hi[2]) == (-32, 1 << 23)                        # +inf clamps to the end of the key range
    assert h.hkf_erase_map_box_voxels(None, None, C.c_float(cell), lo, hi) == -1
