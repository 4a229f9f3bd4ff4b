"""CPU-only: the map's distance field without a device.  The restatement the GPU test compares against (tests/map_edt_expect.py: np_edt, the three windowed
integer passes) is held against the definition -- the brute-force minimum over all sites -- and against scipy's exact Euclidean transform; the sub-box
property is asserted on it; the ABI is exported, bound and declared as include/hybkf.h says and refuses a NULL context writing nothing; the shims answer -1
without an application; host/edt_box_voxels.hpp (metres to box, the radius clamp, the tile plan) runs as a stand-alone program under AddressSanitizer +
UBSan; and every analytic set the GPU test compares holds at least one voxel of each kind that makes the comparison mean something (case_mix)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_edt_expect as E
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1001
BOX = (11, 9, 5)
DENSITIES = (0.0, 0.0005, 0.01, 0.2)
RADII = (1, 3, 7, 12)


def random_sites(density, R, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = BOX
    site = rng.random((nz + 2 * R, ny + 2 * R, nx + 2 * R)) < density
    if density == 0.0005:                                         # so thin a set may be empty: one site in the halo, one in the box
        site[0, 0, 0] = True
        site[R + 2, R + 4, R + 5] = True
    return site


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("density", DENSITIES)
def test_restatement_against_the_definition(density, R):
    site = random_sites(density, R, 100 * R + int(density * 10000))
    got, want = E.np_edt(site, R, BOX), E.np_brute(site, R, BOX)
    assert got.dtype == np.uint16 and np.array_equal(got, want), (density, R, int(np.count_nonzero(got != want)))
    if density == 0.0:
        assert (got == E.FAR).all()
    else:
        assert (got != E.FAR).any()


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("density", DENSITIES[1:])
def test_restatement_against_scipy(density, R):
    ndi = pytest.importorskip("scipy.ndimage")
    site = random_sites(density, R, 7 + 100 * R + int(density * 10000))
    nx, ny, nz = BOX
    d = ndi.distance_transform_edt(~site)                         # the distance to the nearest site of the widened region, fp64
    d2 = np.rint(d * d).astype(np.int64)[R:R + nz, R:R + ny, R:R + nx]
    want = np.where(d2 <= R * R, d2, E.FAR).astype(np.uint16)     # (a voxel within R of a site has that site inside the widened region)
    assert np.array_equal(E.np_edt(site, R, BOX), want)


@pytest.mark.parametrize("R", (3, 7))
def test_sub_box_property(R):
    """the field of an inner box is the same bytes as that part of the field of a box that encloses it"""
    rng = np.random.default_rng(5 + R)
    outer, off, inner = (23, 19, 14), (5, 3, 2), (9, 11, 7)
    site = rng.random((outer[2] + 2 * R, outer[1] + 2 * R, outer[0] + 2 * R)) < 0.004
    whole = E.np_edt(site, R, outer)
    sub = site[off[2]:off[2] + inner[2] + 2 * R, off[1]:off[1] + inner[1] + 2 * R, off[0]:off[0] + inner[0] + 2 * R]
    part = E.np_edt(sub, R, inner)
    assert (whole != E.FAR).any() and (whole == E.FAR).any()
    assert np.array_equal(part, whole[off[2]:off[2] + inner[2], off[1]:off[1] + inner[1], off[0]:off[0] + inner[0]])


def test_classes():
    t = np.array([1.0, 0.5, 0.25, 0.0, -0.25, -1.0, 0.5, np.nan], np.float32)
    w = np.array([1, 1, 1, 2, 1, 9, 0, 1], np.float32)
    assert E.np_classify(t, w, 0.0).tolist() == [1, 1, 1, 2, 2, 2, 0, 2]
    assert E.np_classify(t, w, 0.25).tolist() == [1, 1, 2, 2, 2, 2, 0, 2]
    assert E.np_classify(t, w, -0.25).tolist() == [1, 1, 1, 1, 2, 2, 0, 2]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------
FIELD = ["const int32_t lo_vox[3]", "const uint32_t dims[3]", "uint32_t radius", "float level", "uint32_t site_mask", "uint16_t* %sdist2", "uint8_t* %scls"]


def test_symbols_header_and_binding():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name, prefix in (("kf_map_distance_field", ""), ("kf_map_distance_field_device", "dev_")):
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] == "kf_ctx* ctx" and args[1:] == [a % prefix if "%s" in a else a for a in FIELD], (name, args)
        assert len(getattr(lib, name).argtypes) == len(FIELD) + 1, name
    for name, value in (("KF_VOX_UNKNOWN", "0"), ("KF_VOX_FREE", "1"), ("KF_VOX_OCCUPIED", "2"), ("KF_EDT_FAR", "0xFFFFu")):
        assert re.search(r"^#define %s %s$" % (name, value), header, re.M), name
    assert (K.VOX_UNKNOWN, K.VOX_FREE, K.VOX_OCCUPIED, K.EDT_FAR) == (0, 1, 2, 0xFFFF) == (E.UNKNOWN, E.FREE, E.OCCUPIED, E.FAR)
    for name in ("map_distance_field", "map_distance_field_device"):
        assert hasattr(K.Context, name), name
    assert hasattr(H.App, "distance_field") and hasattr(H.SlabsApp, "distance_field")


def test_null_context_is_refused_without_a_device():
    lib = K.load()
    lo, dims = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(2, 2, 2)
    d, c = np.full(8, 7, np.uint16), np.full(8, 7, np.uint8)
    for fn in (lib.kf_map_distance_field, lib.kf_map_distance_field_device):
        assert fn(None, lo, dims, 3, C.c_float(0.0), 4, K._p(d), K._p(c)) == ARG
        assert fn(None, None, None, 0, C.c_float(float("nan")), 0, None, None) == ARG
    assert (d == 7).all() and (c == 7).all()


def test_shims_without_an_application():
    h = H.load()
    l, u = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    lo, dims, radius = (C.c_int32 * 3)(7, 7, 7), (C.c_uint32 * 3)(7, 7, 7), C.c_uint32(7)
    dist, cls = np.full(8, 7, np.float32), np.full(8, 7, np.uint8)
    for name in ("hkf_app_distance_field", "hkf_app_distance_field_box"):
        assert hasattr(h, name), name
    assert h.hkf_app_distance_field_box(l, u, C.c_float(1.0), lo, dims, C.byref(radius)) == -1
    assert h.hkf_app_distance_field(l, u, C.c_float(1.0), C.c_float(0.0), C.c_uint32(4), C.c_uint64(8), K._p(dist), K._p(cls), lo, dims, C.byref(radius)) == -1
    s = H.load_slabs()
    assert s.hkf_slabs_distance_field(l, u, C.c_float(1.0), C.c_float(0.0), C.c_uint32(4), C.c_uint64(8), K._p(dist), K._p(cls), lo, dims, C.byref(radius)) == -1
    assert (dist == 7).all() and (cls == 7).all() and list(lo) == [7, 7, 7] and list(dims) == [7, 7, 7] and radius.value == 7


def test_box_radius_and_tiles_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_edt_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "host"), "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"),
                           os.path.join(ROOT, "tests", "map_edt_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map edt ok", out.stdout[-3000:]


# ---- the GPU test's sets are not vacuous -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,R,lo,dims", E.analytic_sets())
def test_case_mix_of_the_gpu_sets(kind, R, lo, dims):
    """every kind of voxel in every analytic set: a site, a voxel nearer than R, one at exactly R, one whose nearest site is at R^2 + 1 (FAR), one whose
    nearest site lies outside the box, one whose nearest site is off the box on all three axes -- where R^2 >= 3 allows such an offset at all: with R = 1
    the only offsets within the radius are along one axis --, and a tie between two sites"""
    mix = E.case_mix(E.analytic_map(kind, R, lo, dims), lo, dims, R)
    print(kind, R, mix)
    for k in ("zero", "inside", "exact", "far_by_one", "halo", "tie"):
        if k == "inside" and R == 1:
            continue                                              # (0 < d2 < 1 has no integer)
        if k == "zero" and R == 255:
            continue                                              # (a site inside the box of 9 voxels would leave nothing at R or beyond: special_sites)
        assert mix[k] >= 1, (kind, R, k, mix)
    if R * R >= 3:
        assert mix["diagonal"] >= 1, (kind, R, mix)
    # the special sites are where special_sites puts them: R^2 from the low corner with no nearer site, the pair around its middle voxel
    if kind == "single":
        d2, _ = E.expected(E.analytic_map(kind, R, lo, dims), lo, dims, R)
        assert d2[0, 0, 0] == R * R
        if R == 255:
            assert d2[8, 8, 8] == 250 * 250 and d2[8, 7, 3] == E.FAR and d2[8, 8, 3] == R * R
        else:
            gap = 1 if R == 1 else 2
            assert d2[-2, -2, -1 - gap] == gap * gap


def test_empty_map_is_all_far():
    d2, cls = E.expected(E.analytic_map("empty", 7), E.BOX_LO, E.BOX_DIMS, 7)
    assert (d2 == E.FAR).all() and (cls == E.UNKNOWN).all()
    d2, _ = E.expected({}, E.BOX_LO, E.BOX_DIMS, 7, site_mask=1 << E.UNKNOWN)
    assert (d2 == 0).all()
