"""CPU-only: the moving volume's ABI (kf_shift_volume, kf_volume_origin) is exported and refuses a NULL context; the host arithmetic that
decides when and how far HybKinectfu::processNewFrame shifts (hkf_recentre_shift) agrees with a numpy fp32 restatement; and the same code
passes a stand-alone AddressSanitizer + UBSan run."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_symbols_exported():
    lib = K.load()
    assert hasattr(lib, "kf_shift_volume") and hasattr(lib, "kf_volume_origin")
    assert "kf_shift_volume" in K.SYMBOLS and "kf_volume_origin" in K.SYMBOLS
    h = H.load()
    for name in ("hkf_recentre_shift", "hkf_world_pose", "hkf_world_positions", "hkf_app_shift_volume", "hkf_app_volume_origin", "hkf_app_set_recentre"):
        assert hasattr(h, name), name


def test_null_context_is_an_argument_error():
    lib = K.load()
    assert lib.kf_shift_volume(None, 0, 0, 0) == 1001
    assert lib.kf_shift_volume(None, 8, 0, 0) == 1001
    o = (C.c_int32 * 3)()
    assert lib.kf_volume_origin(None, o) == 1001


def expected_shift(pose, size, res, dist):
    """hkf_recentre_shift in numpy fp32, one rounding per operation"""
    pose = np.asarray(pose, f32)
    half = f32(size) * f32(0.5)
    step = f32(8) * (f32(size) / f32(res))
    off = [(pose[i, 3] + pose[i, 2] * half) - half for i in range(3)]
    assert all(type(o) is np.float32 for o in off)
    if not (dist > 0) or not any(abs(o) > f32(dist) for o in off):
        return (0, 0, 0)
    return tuple(int(np.trunc(o / step)) * 8 for o in off)


def yaw(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    r = np.eye(4, dtype=np.float64)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = c, s, -s, c
    return r


def test_recentre_shift_matches_numpy():
    size, res = 2.0, 64                                           # cell 1 / 32, a brick 0.25 m
    p0 = S.pose0(size)

    def at(x, y, z, rot=None):
        p = np.eye(4) if rot is None else rot.copy()
        p[:3, 3] = (x, y, z)
        return p.astype(f32)

    cases = [
        (p0, 0.5, (0, 0, 0)),                                     # inside the threshold
        (p0, 0.0, (0, 0, 0)),                                     # the policy is off
        (at(1.51, 1.0, -0.3), 0.5, (16, 0, -8)),                  # just outside on x: every axis moves by its own whole bricks
        (at(1.49, 1.0, -0.3), 0.5, (0, 0, 0)),                    # just inside
        (at(0.3, 1.0, -0.3), 0.5, (-16, 0, -8)),                  # -2.8 bricks truncate toward zero: -2, not -3
        (at(1.0, 1.0, 0.3, yaw(90)), 0.5, (32, 0, -16)),          # the camera looks along +x: the focus point lies 1 m from it along x, at its own z
        (at(1.0, 1.0, -0.3, yaw(30)), 0.2, None),                 # a rotated camera near the threshold: whatever numpy says
        (at(1.2, 0.4, 0.1, yaw(-50)), 0.3, None),
    ]
    for pose, dist, want in cases:
        got = H.recentre_shift(pose, size, res, dist)
        assert got == expected_shift(pose, size, res, dist), (pose, dist, got)
        if want is not None:
            assert got == want, (pose, dist, got)
        assert all(g % 8 == 0 for g in got)
    # the 2 cm circle of Scene S never triggers at 0.35 m, at either test volume
    for size, res in ((2.0, 64), (4.0, 128)):
        for k in range(0, 100, 7):
            assert H.recentre_shift(S.trajectory_pose(k, size), size, res, 0.35) == (0, 0, 0)


def test_host_arithmetic_under_sanitizers(tmp_path):
    """recentre.cpp + a main of its own, -fsanitize=address,undefined, run on the CPU: nothing is loaded into Python"""
    host = os.path.join(ROOT, "hybkinectfu_amd", "host")
    exe = str(tmp_path / "shift_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fsanitize=float-cast-overflow", "-ffp-contract=off", "-I", host, os.path.join(ROOT, "tests", "shift_host_main.cpp"),
                           os.path.join(host, "recentre.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "shift host arithmetic ok" in out.stdout, out.stdout
