"""CPU-only: the ABI of the map queries.  kf_map_sample, kf_map_sample_device, kf_map_cast_rays and kf_map_cast_rays_device are exported, bound, declared
with the argument counts of include/hybkf.h and refuse a NULL context without a device, writing nothing; the host shim's names and the Python methods exist
and answer -1 without an application; the slab shim always answers -1.  hkf_map_query_voxels (no application, no device) states the metres -> voxels rule."""
import ctypes as C
import os
import re

import numpy as np

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1001
SAMPLE = ["uint32_t n", "const double* %spos", "float* %stsdf", "float* %sweight", "float* %sgrad", "uint8_t* %scolor"]
CAST = ["uint32_t n", "const double* %sorigin", "const float* %sdir", "const float* %stmin", "const float* %stmax", "float step", "uint32_t max_steps",
        "uint8_t* %sstatus", "float* %st", "float* %snormal", "uint8_t* %scolor", "float* %sweight"]


def declared_args(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def fill(names, prefix):
    return [a % prefix if "%s" in a else a for a in names]


def test_symbols_header_and_binding():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name, want in (("kf_map_sample", fill(SAMPLE, "")), ("kf_map_sample_device", fill(SAMPLE, "dev_")), ("kf_map_cast_rays", fill(CAST, "")),
                       ("kf_map_cast_rays_device", fill(CAST, "dev_"))):
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        args = declared_args(header, name)
        assert args[0] == "kf_ctx* ctx" and args[1:] == want, (name, args)
        assert len(getattr(lib, name).argtypes) == len(want) + 1, name
    for name, value in (("KF_RAY_MISS", 0), ("KF_RAY_HIT", 1), ("KF_RAY_BROKEN", 2)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M), name
    assert (K.RAY_MISS, K.RAY_HIT, K.RAY_BROKEN) == (0, 1, 2)
    for name in ("map_sample", "map_sample_device", "map_cast_rays", "map_cast_rays_device"):
        assert hasattr(K.Context, name), name
    for name in ("sample_map", "cast_map_rays"):
        assert hasattr(H.App, name) and hasattr(H.SlabsApp, name), name


def test_null_context_is_refused_without_a_device():
    lib = K.load()
    pos = np.full((4, 3), 1.5, np.float64)
    d = np.ones((4, 3), np.float32)
    t0, t1 = np.zeros(4, np.float32), np.full(4, 9, np.float32)
    f4, f12, b4, b16 = np.full(4, 7, np.float32), np.full(12, 7, np.float32), np.full(4, 7, np.uint8), np.full(16, 7, np.uint8)
    p = K._p
    for fn in (lib.kf_map_sample, lib.kf_map_sample_device):
        assert fn(None, 4, p(pos), p(f4), p(f4), p(f12), p(b16)) == ARG
        assert fn(None, 0, None, None, None, None, None) == ARG
    for fn in (lib.kf_map_cast_rays, lib.kf_map_cast_rays_device):
        assert fn(None, 4, p(pos), p(d), p(t0), p(t1), 0.5, 100, p(b4), p(f4), p(f12), p(b16), p(f4)) == ARG
        assert fn(None, 4, p(pos), p(d), p(t0), p(t1), float("nan"), 0, None, None, None, None, None) == ARG
    assert (f4 == 7).all() and (f12 == 7).all() and (b4 == 7).all() and (b16 == 7).all()       # refused: nothing written


def test_shims_without_an_application():
    h = H.load()
    pos = np.full((2, 3), 0.5, np.float64)
    d = np.ones((2, 3), np.float32)
    t = np.zeros(2, np.float32)
    out = np.full(2, 7, np.float32)
    p = K._p
    for name in ("hkf_app_sample_map", "hkf_app_cast_map_rays", "hkf_map_query_voxels"):
        assert hasattr(h, name), name
    assert h.hkf_app_sample_map(p(pos), C.c_uint32(2), p(out), None, None, None) == -1
    assert h.hkf_app_cast_map_rays(p(pos), p(d), p(t), p(t), C.c_uint32(2), None, p(out), None, None, None) == -1
    s = H.load_slabs()
    assert s.hkf_slabs_sample_map(p(pos), C.c_uint32(2), p(out), None, None, None) == -1
    assert s.hkf_slabs_cast_map_rays(p(pos), p(d), p(t), p(t), C.c_uint32(2), None, p(out), None, None, None) == -1
    assert (out == 7).all()


def test_metres_to_voxels_is_one_fp64_division():
    """cell 3 / 512 as the fp32 quotient: the position in voxels is x / (double)cell, so voxel g's centre (g + 1/2) * cell lands within rounding of g + 1/2"""
    h = H.load()
    cell = np.float32(3.0) / np.float32(512)
    rng = np.random.default_rng(2)
    m = np.concatenate([rng.uniform(-40, 40, 61), [0.0, float(cell), -2.5 * float(cell)]]).reshape(-1, 1).repeat(3, axis=1).copy()
    vox = np.zeros_like(m)
    assert h.hkf_map_query_voxels(K._p(m), C.c_uint32(m.size), C.c_float(cell), K._p(vox)) == 0
    assert np.array_equal(vox, m / np.float64(cell))
    assert vox[-3, 0] == 0.0 and vox[-2, 0] == 1.0 and vox[-1, 0] == -2.5
    assert h.hkf_map_query_voxels(None, C.c_uint32(3), C.c_float(cell), K._p(vox)) == -1
