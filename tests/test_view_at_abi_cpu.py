"""CPU-only: the map viewer's ABI (kf_render_view_at) is exported, bound and declared, and refuses a NULL context; the host arithmetic that places the
window for a view of the map (hkf_view_frame) agrees with a numpy fp32 restatement and with hkf_recentre_shift; and the same code passes a
stand-alone AddressSanitizer + UBSan run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_symbol_exported_bound_and_declared():
    lib = K.load()
    assert hasattr(lib, "kf_render_view_at") and "kf_render_view_at" in K.SYMBOLS
    assert lib.kf_render_view_at.argtypes is not None and len(lib.kf_render_view_at.argtypes) == 10
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    decl = re.search(r"\bint\s+kf_render_view_at\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/hybkf.h does not declare kf_render_view_at"
    assert len(decl.group(1).split(",")) == 10 and "frame_origin_vox[3]" in decl.group(1)
    declared = set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", header))
    assert set(K.SYMBOLS) <= declared, sorted(set(K.SYMBOLS) - declared)
    assert hasattr(K.Context, "render_view_at")
    h = H.load()
    for name in ("hkf_view_frame", "hkf_app_render_view_at", "hkf_app_render_map_view"):
        assert hasattr(h, name), name
    assert hasattr(H.App, "render_view_at") and hasattr(H.App, "render_map_view")


def test_null_context_is_an_argument_error():
    lib = K.load()
    frame = (C.c_int32 * 3)(0, 0, 0)
    cam = K.camera(160, 120, 79.5, 59.5, 131.25, 131.25)
    rp = K.RaycastParams(0.1)
    for mode in (K.VIEW_NORMALS, K.VIEW_COLOR, 7):
        assert lib.kf_render_view_at(None, mode, frame, None, C.byref(cam), C.byref(rp), C.c_float(0.1), C.c_float(4.0), None, None) == 1001
    assert lib.kf_render_view_at(None, 0, None, None, None, None, C.c_float(0.1), C.c_float(4.0), None, None) == 1001


def expected_frame(pose, size, res):
    """hkf_view_frame in numpy fp32, one rounding per operation, in its order"""
    pose = np.asarray(pose, f32)
    half = f32(size) * f32(0.5)
    cell = f32(size) / f32(res)
    step = f32(8) * cell
    with np.errstate(all="ignore"):
        off = [(pose[i, 3] + pose[i, 2] * half) - half for i in range(3)]
        assert all(type(o) is np.float32 for o in off)
        if not all(abs(o) <= f32(3.0e38) for o in off):
            return (0, 0, 0), pose.copy()
        q = [min(max(np.trunc(o / step), f32(-1.0e6)), f32(1.0e6)) for o in off]
    frame = tuple(int(x) * 8 for x in q)
    local = pose.copy()
    for i in range(3):
        local[i, 3] = pose[i, 3] - f32(frame[i]) * cell
    return frame, local


def same(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def random_pose(rng, spread):
    p = np.eye(4)
    p[:3, :3] = rotation(rng)
    p[:3, 3] = rng.uniform(-spread, spread, 3)
    return p.astype(f32)


def test_view_frame_matches_numpy():
    rng = np.random.default_rng(20240611)
    n = 0
    for size, res in ((2.0, 64), (2.25, 72), (3.0, 128), (4.0, 512)):
        for spread in (1.0, 10.0, 300.0):
            for _ in range(30):
                pose = random_pose(rng, spread)
                frame, local = H.view_frame(pose, size, res)
                want_frame, want_local = expected_frame(pose, size, res)
                assert frame == want_frame and same(local, want_local), (size, res, pose, frame, want_frame)
                assert all(f % 8 == 0 for f in frame)
                assert same(local[:, :3], pose[:, :3]) and same(local[3], pose[3])
                n += 1
    assert n == 360


def at(x, y, z):
    p = np.eye(4, dtype=f32)
    p[:3, 3] = (x, y, z)
    return p


def test_view_frame_clamp_and_poses_that_are_not_finite():
    size, res = 2.0, 64
    for x, want in ((1.0e30, 8000000), (-1.0e30, -8000000), (3.0e38, 8000000), (2.6e5, 8000000), (-2.6e5, -8000000)):
        frame, local = H.view_frame(at(x, 1.0, -0.3), size, res)
        assert frame == (want, 0, -8) and frame == expected_frame(at(x, 1.0, -0.3), size, res)[0], (x, frame)
    for bad in (np.nan, np.inf, -np.inf):
        for where in ((0, 3), (1, 3), (2, 3), (0, 2), (2, 2)):
            pose = at(1.7, 1.0, -0.3)
            pose[where] = bad
            frame, local = H.view_frame(pose, size, res)
            assert frame == (0, 0, 0) and same(local, pose), (bad, where, frame)
    for size_bad, res_bad in ((0.0, 64), (-1.0, 64), (2.0, 0)):
        pose = at(5.3, 1.0, -2.0)
        frame, local = H.view_frame(pose, size_bad, res_bad)
        assert frame == (0, 0, 0) and same(local, pose)


def test_view_frame_is_zero_within_one_brick_of_the_centre():
    size, res = 2.0, 64                                           # a brick is 0.25 m; the focus of an identity rotation is t + (0, 0, 1)
    rng = np.random.default_rng(7)
    for _ in range(50):
        off = rng.uniform(-0.249, 0.249, 3)
        pose = at(1.0 + off[0], 1.0 + off[1], 0.0 + off[2])
        frame, local = H.view_frame(pose, size, res)
        assert frame == (0, 0, 0) and same(local, pose), (off, frame)
    assert H.view_frame(at(1.26, 1.0, 0.0), size, res)[0] == (8, 0, 0)
    assert H.view_frame(at(1.0, 0.74, 0.0), size, res)[0] == (0, -8, 0)


def test_view_frame_is_the_shift_recentring_would_make():
    """for a pose that makes hkf_recentre_shift move the window by s from origin 0, the frame is s: the window recentring would leave behind"""
    rng = np.random.default_rng(11)
    moved = 0
    for size, res in ((2.0, 64), (3.0, 128)):
        for _ in range(100):
            pose = random_pose(rng, 3.0)
            pose[:3, 3] += f32(size / 2)
            s = H.recentre_shift(pose, size, res, 0.35)
            if s == (0, 0, 0):
                continue
            moved += 1
            assert H.view_frame(pose, size, res)[0] == s, (pose, s)
    assert moved >= 100, moved


def test_view_frame_under_sanitizers(tmp_path):
    """recentre.cpp + a main of its own, -fsanitize=address,undefined, run on the CPU: nothing is loaded into Python"""
    host = os.path.join(ROOT, "hybkinectfu_amd", "host")
    exe = str(tmp_path / "view_at_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fsanitize=float-cast-overflow", "-ffp-contract=off", "-I", host, os.path.join(ROOT, "tests", "view_at_host_main.cpp"),
                           os.path.join(host, "recentre.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "view frame arithmetic ok" in out.stdout, out.stdout
