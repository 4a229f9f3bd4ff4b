"""CPU-only: the ABI and the host side of merging maps under a rigid transform.  kf_merge_brick_store_rigid and kf_rigid_brick_keys are exported, bound,
declared and refuse what they must without a device; the host shim's names and the Python methods exist and answer -1 without an application; the slab shim
always answers -1.  kf_rigid_brick_keys is compared with a numpy float64 restatement of its rule (include/hybkf.h), operation for operation.  The header the
library's host side lives in (csrc/rigid_keys.h) also runs in a stand-alone program with a main of its own (tests/map_resample_main.cpp), built with
AddressSanitizer + UBSan: nothing of it is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HI = (1 << 20) - 1


def rotation(deg, axis, t):
    """Rodrigues, float64: the 3x4 [R | t]"""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    r = np.cos(a) * np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * np.outer(k, k)
    return np.concatenate([r, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def quarter_turn_z(t):
    """exactly a signed permutation: x -> y, y -> -x"""
    return np.array([[0, -1, 0, t[0]], [1, 0, 0, t[1]], [0, 0, 1, t[2]]], np.float64)


def np_candidates(keys, xf):
    """the rule of kf_rigid_brick_keys: per source brick the 8 corners p of [8k - 1, 8k + 8]^3, d_i = (((R[i][0] (p_0 + .5) + R[i][1] (p_1 + .5)) + R[i][2]
    (p_2 + .5)) + t_i) - .5 in float64, the bricks of floor(min) .. ceil(max); unique, sorted by (z, y, x)"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    xf = np.asarray(xf, np.float64)
    out = set()
    for k in keys:
        d = np.empty((8, 3))
        for c in range(8):
            p = np.array([8.0 * k[j] + (8.0 if (c >> j) & 1 else -1.0) + 0.5 for j in range(3)])
            for i in range(3):
                d[c, i] = (((xf[i, 0] * p[0] + xf[i, 1] * p[1]) + xf[i, 2] * p[2]) + xf[i, 3]) - 0.5
        b0 = np.floor(d.min(axis=0)).astype(np.int64) >> 3
        b1 = np.ceil(d.max(axis=0)).astype(np.int64) >> 3
        for z in range(b0[2], b1[2] + 1):
            for y in range(b0[1], b1[1] + 1):
                for x in range(b0[0], b1[0] + 1):
                    out.add((x, y, z))
    return np.array(sorted(out, key=lambda k: (k[2], k[1], k[0])), np.int32).reshape(-1, 3)


def source_keys():
    """a blob of bricks, a lone one, and negative coordinates"""
    rng = np.random.default_rng(3)
    blob = {(x, y, z) for z in range(-2, 2) for y in range(0, 3) for x in range(-1, 4) if rng.random() < 0.7}
    blob |= {(9, -7, 5), (-12, 0, 0)}
    return np.array(sorted(blob), np.int32)


TRANSFORMS = {
    "identity": rotation(0, (0, 0, 1), (0, 0, 0)),
    "bricks": rotation(0, (0, 0, 1), (8, -16, 24)),
    "quarter_z": quarter_turn_z((3, -5, 12)),
    "oblique": rotation(20, (1, 2, 3), (2.3, -1.7, 0.4)),
}


def raw_keys(keys, xf, out, cap):
    lib = K.load()
    return lib.kf_rigid_brick_keys(len(keys), K._p(keys) if keys is not None else None, K.rigid_xf(xf) if xf is not None else None,
                                   K._p(out) if out is not None else None, cap)


def test_symbols_exported_bound_and_declared():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name in ("kf_merge_brick_store_rigid", "kf_rigid_brick_keys"):
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"^int kf_merge_brick_store_rigid\(kf_ctx\* ctx", header, re.M)
    assert re.search(r"^int64_t kf_rigid_brick_keys\(uint32_t count", header, re.M)
    assert len(lib.kf_merge_brick_store_rigid.argtypes) == 7 and len(lib.kf_merge_brick_store.argtypes) == 7
    assert len(lib.kf_rigid_brick_keys.argtypes) == 5 and lib.kf_rigid_brick_keys.restype is C.c_int64
    assert hasattr(K.Context, "merge_brick_store_rigid") and hasattr(K, "rigid_brick_keys")
    assert "is not offered" not in header                         # the sentence that admitted the gap points to the new entry


def test_null_arguments():
    lib = K.load()
    keys, t, w = np.zeros((1, 3), np.int32), np.zeros(512, np.float32), np.ones(512, np.float32)
    xf = K.rigid_xf(TRANSFORMS["identity"])
    assert lib.kf_merge_brick_store_rigid(None, 1, K._p(keys), K._p(t), K._p(w), None, xf) == 1001
    assert lib.kf_merge_brick_store_rigid(None, 0, None, None, None, None, None) == 1001
    assert lib.kf_rigid_brick_keys(1, None, xf, None, 0) == -1
    assert lib.kf_rigid_brick_keys(1, K._p(keys), None, None, 0) == -1
    assert lib.kf_rigid_brick_keys(1, K._p(keys), xf, None, 3) == -1
    assert lib.kf_rigid_brick_keys(0, None, xf, None, 0) == 0


def test_shims_without_an_application():
    h = H.load()
    m = np.eye(4, dtype=np.float32)
    assert hasattr(h, "hkf_app_merge_map_rigid") and h.hkf_app_merge_map_rigid(b"/nonexistent/x", m.ctypes.data_as(C.c_void_p)) == -1
    s = H.load_slabs()                                            # the slab class refuses: the store stays a single-GPU feature
    assert hasattr(s, "hkf_slabs_merge_map_rigid") and s.hkf_slabs_merge_map_rigid(b"/nonexistent/x", m.ctypes.data_as(C.c_void_p)) == -1
    assert hasattr(H.App, "merge_map_rigid") and hasattr(H.SlabsApp, "merge_map_rigid")


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_candidates_against_numpy(name):
    keys, xf = source_keys(), TRANSFORMS[name]
    want = np_candidates(keys, xf)
    got = K.rigid_brick_keys(keys, xf)
    assert np.array_equal(got, want), name
    o = np.lexsort((got[:, 0], got[:, 1], got[:, 2]))
    assert np.array_equal(o, np.arange(len(got))) and len({tuple(k) for k in got.tolist()}) == len(got)      # sorted (z, y, x), unique
    # cap: the count is the whole list's, only the first `cap` are written
    few = np.full((6, 3), 0x55555555, np.int32)
    assert raw_keys(keys, xf, few, 5) == len(want) and np.array_equal(few[:5], want[:5]) and np.all(few[5] == 0x55555555)
    have = {tuple(k) for k in got.tolist()}
    if name == "identity":                                        # every source key and its 26 neighbours: the +-1-voxel reach
        for k in keys.tolist():
            for z in (-1, 0, 1):
                for y in (-1, 0, 1):
                    for x in (-1, 0, 1):
                        assert (k[0] + x, k[1] + y, k[2] + z) in have, k
        assert len(have) == len({(k[0] + x, k[1] + y, k[2] + z) for k in keys.tolist() for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)})
    if name == "bricks":
        assert np.array_equal(got, K.rigid_brick_keys(keys, TRANSFORMS["identity"]) + np.array([1, -2, 3], np.int32))
    # never too few: the brick of every transformed source voxel centre, and of its neighbours one voxel away, is a candidate
    r, t = xf[:, :3], xf[:, 3]
    g = np.arange(-1, 9, dtype=np.float64)
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    local = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    for k in keys.tolist():
        d = (local + 8.0 * np.array(k) + 0.5) @ r.T + t - 0.5
        for b in {tuple(v) for v in np.floor(d / 8.0).astype(np.int64).tolist()}:
            assert b in have, (k, b)


def test_refusals():
    keys = source_keys()
    xf = TRANSFORMS["oblique"]
    assert raw_keys(keys, xf, None, 0) > 0
    for i in range(12):
        for v in (np.nan, np.inf):
            bad = xf.copy()
            bad.reshape(-1)[i] = v
            assert raw_keys(keys, bad, None, 0) == -1, i
    scaled = xf.copy()
    scaled[:, :3] *= 1.001
    assert raw_keys(keys, scaled, None, 0) == -1
    mirror = xf.copy()
    mirror[0, :3] *= -1                                           # orthonormal, det -1
    assert abs(np.linalg.det(mirror[:, :3]) + 1) < 1e-12 and raw_keys(keys, mirror, None, 0) == -1
    f32 = xf.astype(np.float32).astype(np.float64)               # a rotation rounded to fp32 is accepted
    assert raw_keys(keys, f32, None, 0) > 0
    # a translation that pushes a candidate past 2^20: the largest source x is 9, its candidates reach brick 10
    fits = rotation(0, (0, 0, 1), (8.0 * (HI - 10), 0, 0))
    past = rotation(0, (0, 0, 1), (8.0 * (HI - 9), 0, 0))
    assert raw_keys(keys, fits, None, 0) > 0 and raw_keys(keys, past, None, 0) == -1
    assert raw_keys(keys, rotation(0, (0, 0, 1), (0, -1e300, 0)), None, 0) == -1
    with pytest.raises(K.KfError):
        K.rigid_brick_keys(keys, past)


def test_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_resample_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "map_resample_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map resample ok", out.stdout[-3000:]
