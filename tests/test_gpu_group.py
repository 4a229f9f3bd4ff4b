"""GPU: slab groups (include/hybkf_group.h) reproduce the whole-volume context bit for bit -- poses after every frame, merged model maps
(levels 0-2), owned TSDF layers, observed-voxel counts, the marching-cubes triangle sequence -- on one device (LOCAL, up to the full-size
8-way C4 geometry), over RCCL (in child processes), through a lost frame, and through the C++ class HybKinectfuSlabs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hybkinectfu_amd import group as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import pipeline as PL
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = S.STOCK
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]


@pytest.fixture(autouse=True)
def _close_leaked_groups():
    """a failed test leaves its group (and its member contexts) alive in the traceback: close it, or the persistent tracking loops stay
    off for every later test in the process"""
    yield
    for g in G.live_groups():
        g.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def whole_frame(ctx, mm, k, trunc_max=P["depth_trunc_max"], integ_dist=P["integrate_depth_trunc"]):
    """the whole-volume context through the calls a group member makes, kf_raycast_volume in place of the slab merge"""
    if isinstance(mm, np.ndarray):
        ctx.upload_depth_mm(mm)
    else:
        ctx.set_depth_mm_device(mm)
    ctx.preprocess(P["depth_trunc_min"], trunc_max, P["filter_sigma_pixel"], P["filter_sigma_depth"])
    ctx.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
    ctx.integrate(None, P["integrate_sdf_trunc"], integ_dist)
    ctx.raycast(None, INC, P["depth_trunc_min"], trunc_max)


def check_frame(g, whole, k, tracked=True):
    ok_g, pose_g, st_g, _ = g.track_result(check_lockstep=True)          # (every member: the same pose bits, verdict, status, fused / lost)
    ok_w, pose_w, st_w, _ = whole.track_result()
    assert ok_g == ok_w == tracked and st_g == st_w, (k, ok_g, ok_w, st_g, st_w)
    assert np.array_equal(bits(pose_g), bits(pose_w)), k
    for i, m in enumerate(g.members()):
        ok_m, pose_m, st_m, _ = m.track_result()
        assert ok_m == ok_g and st_m == st_g and np.array_equal(bits(pose_m), bits(pose_w)), (k, i)
        for level in range(3):
            for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                assert np.array_equal(bits(m.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (k, i, level, map_id)


def check_volume(g, whole):
    tw, ww = whole.download_volume()
    for m in g.members():
        z0, z1 = m.owned
        t, w = m.download_volume(z0, z1)
        assert np.array_equal(bits(t), bits(tw[z0:z1])) and np.array_equal(w, ww[z0:z1]), (z0, z1)
    assert sum(m.stats()["weight_gt0"] for m in g.members()) == whole.stats()["weight_gt0"] == int((ww > 0).sum())


def _probe_cuts(res, size, world):
    cam = S.vga_camera()
    first = torch.from_numpy(S.render_depth_mm(S.trajectory_pose(0, size), cam, size).astype(np.int16)).cuda()
    work = PL.probe_layer_work(K.camera(*cam), res, size, None, first.data_ptr(), probe_res=64)
    halo = PL.slab_halo_layers(res, size, INC)
    ranges = PL.slab_ranges(res, world, work, halo=halo)
    assert ranges != PL.slab_ranges(res, world)                    # the probe moved the boundaries
    return [0] + [r[1] for r in ranges]


@pytest.mark.parametrize("cuts", [[0, 40, 192], [0, 64, 128, 192], "probe4"], ids=["uneven2", "even3", "probe4"])
def test_local_group_equals_whole_volume(cuts):
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    if cuts == "probe4":
        cuts = _probe_cuts(res, size, 4)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, max_triangles=600000)
    whole.set_pose(S.pose0(size))
    g = G.Group.local(kcam, res, size, cuts, max_triangles=600000)
    assert g.halo == PL.slab_halo_layers(res, size, INC) and len(g.members()) == len(cuts) - 1
    for k in range(6):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        whole_frame(whole, mm, k)
        g.frame(mm, k)                                             # host frame: one copy into the group's buffer
        check_frame(g, whole, k)
        if k == 0:
            assert int((whole.download_map(K.MAP_MODEL_VERTICES)[..., 3] != 0).sum()) > 10000
    check_volume(g, whole)
    thr = 300 * size / res
    whole.marching_cubes(thr)
    g.marching_cubes(thr)
    wt, gt = whole.triangles(), g.triangles()
    assert len(wt) > 1000 and gt.tobytes() == wt.tobytes()
    # a window across a member boundary (with triangles on both sides) reads the same triangles as the whole context
    ends = np.cumsum([m.triangles().shape[0] for m in g.members()])
    inner = [int(e) for e in ends[:-1] if 5 <= e <= len(wt) - 5]
    win = np.zeros(10, dtype=K.TRI_DTYPE)
    for e in inner:                                                # ([0, 40, 192]: member 0 holds no surface)
        assert G.load().kf_group_read_triangles(g.h, win.ctypes.data_as(C.c_void_p), e - 5, 10) == 0
        assert win.tobytes() == wt[e - 5:e + 5].tobytes()
    assert G.load().kf_group_read_triangles(g.h, win.ctypes.data_as(C.c_void_p), len(wt) - 5, 10) == G.ERR_ARG     # past the end
    g.close()
    whole.close()


def test_c4_eight_members_full_size_on_one_gpu():
    """the 8-way C4 slab geometry at full size: 1024^3 @ 6 m, a slab every 128 layers, halo 8 -- ~9.7 GB of slabs beside the 8.6 GB whole volume"""
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size, gate = 1024, 6.0, 6.0
    params = G.stock_params(trunc_max=gate, integ_dist=gate)
    assert PL.slab_halo_layers(res, size, INC) == 8
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3)
    whole.set_pose(S.pose0(size))
    g = G.Group.local(kcam, res, size, list(range(0, res + 1, 128)), halo=8, params=params)
    assert [m.stored for m in g.members()] == [(max(0, z - 8), min(res, z + 136)) for z in range(0, res, 128)]
    crossings = [0] * 8
    for k in range(3):
        mm = torch.from_numpy(S.render_depth_mm(S.trajectory_pose(k, size), cam, size).astype(np.int16)).cuda()
        whole_frame(whole, mm.data_ptr(), k, gate, gate)
        g.frame(mm.data_ptr(), k)
        check_frame(g, whole, k)
        g.sync()
        torch.cuda.synchronize()
    # the members split the crossings between them: every pixel of the merged map is some member's crossing, and the members that meet any
    # form one run over the layers that hold Scene S (nothing lies in the first 128 layers, 0.75 m, in front of the sphere)
    lib = K.load()
    any_cross = torch.zeros((cam[1], cam[0]), dtype=torch.bool, device="cuda")
    for i, m in enumerate(g.members()):
        ta = torch.empty((cam[1], cam[0]), dtype=torch.int64, device="cuda")
        own = torch.empty_like(ta)
        spec = torch.empty((cam[1], cam[0], 3), dtype=torch.float32, device="cuda")
        assert lib.kf_raycast_volume_slab_cross_spec(m.h, None, C.byref(K.RaycastParams(INC)), C.byref(kcam), C.c_float(P["depth_trunc_min"]),
                                                     C.c_float(gate), C.c_void_p(ta.data_ptr()), C.c_void_p(own.data_ptr()),
                                                     C.c_void_p(spec.data_ptr())) == 0
        g.sync()
        hit = (ta >> 32) != 0x7F800000                             # +inf << 32: no crossing in this member's layers
        crossings[i] = int(hit.sum())
        any_cross |= hit
    wv = whole.download_map(K.MAP_MODEL_VERTICES)
    valid = torch.from_numpy(wv[..., 3] != 0).cuda()
    assert int(valid.sum()) > 10000 and bool((any_cross | ~valid).all()), crossings
    on = [i for i, c in enumerate(crossings) if c > 0]
    assert len(on) >= 4 and on == list(range(on[0], on[-1] + 1)) and crossings[0] == 0, crossings
    # the planes around three member boundaries are bit-equal to the whole volume's
    observed = 0
    for z0, z1 in ((120, 136), (504, 520), (888, 904)):
        tw, ww = whole.download_volume(z0, z1)
        observed += int((ww > 0).sum())
        for m in g.members():
            a, b = max(z0, m.owned[0]), min(z1, m.owned[1])
            if a < b:
                t, w = m.download_volume(a, b)
                assert np.array_equal(bits(t), bits(tw[a - z0:b - z0])) and np.array_equal(w, ww[a - z0:b - z0]), (m.owned, a, b)
    assert observed > 0
    g.close()
    whole.close()


def test_lost_frame_keeps_the_members_in_lock_step():
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3)
    whole.set_pose(S.pose0(size))
    g = G.Group.local(kcam, res, size, [0, 72, 192])
    zero = np.zeros((cam[1], cam[0]), np.uint16)
    seq = [S.render_depth_mm(S.trajectory_pose(k, size), cam, size) for k in range(3)] + [zero] + \
          [S.render_depth_mm(S.trajectory_pose(k, size), cam, size) for k in range(3, 5)]
    for k, mm in enumerate(seq):
        if k == 3:
            before = [(m.stats(), m.download_volume()) for m in g.members()]
        whole_frame(whole, mm, k)
        g.frame(mm, k)
        check_frame(g, whole, k, tracked=(k != 3))
        if k == 3:
            for m, (st0, (t0, w0)) in zip(g.members(), before):
                st = m.stats()
                assert st["frames_lost"] == st0["frames_lost"] + 1 and st["frames_fused"] == st0["frames_fused"], (st0, st)
                t, w = m.download_volume()
                assert np.array_equal(bits(t), bits(t0)) and np.array_equal(w, w0)
            assert whole.stats()["frames_lost"] == 1
    check_volume(g, whole)
    g.close()
    whole.close()


def _child(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k == "KF_STATS_CROSSCHECK"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_rccl_child.py"), mode], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "group rccl ok" in r.stdout, "child %s exited with %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_rccl_all_world1_equals_plain_context():
    _child("all1")


def test_rccl_rank_world1_equals_plain_context():
    _child("rank1")


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason="needs two or more visible devices")
def test_rccl_all_over_every_visible_device():
    _child("alldev")


def test_cpp_slab_class_equals_hybkinectfu(tmp_path):
    """HybKinectfuSlabs (LOCAL, 2 members) through hkf_slabs_* against HybKinectfu through hkf_app_*: pose bits after every frame, the
    saveMesh .ply files byte for byte"""
    cam = S.vga_camera()
    res, size = 192, 3.0
    app = H.App(res, size, cam, max_triangles=600000)
    sl = C.CDLL(os.path.join(K.PKG_DIR, "libhybkf_slabs.so"))
    cuts = (C.c_uint32 * 3)(0, 96, 192)
    assert sl.hkf_slabs_init(res, C.c_float(size), cam[0], cam[1], C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                             600000, C.c_float(0), C.c_float(0), C.c_float(0), 0, G.LOCAL, 2, cuts, None, 0) == 0
    try:
        for k in range(5):
            mm = np.ascontiguousarray(S.render_depth_mm(S.trajectory_pose(k, size), cam, size), np.uint16)
            assert app.process_frame(mm, k)
            assert sl.hkf_slabs_process_frame(mm.ctypes.data_as(C.c_void_p), 0, k) == 1
            ok_a, pa = app.pose()
            ps = np.zeros(16, np.float32)
            assert ok_a and sl.hkf_slabs_get_pose(ps.ctypes.data_as(C.c_void_p)) == 1
            assert np.array_equal(bits(ps.reshape(4, 4)), bits(pa)), k
        n = app.generate_mesh()
        assert n > 1000 and sl.hkf_slabs_generate_mesh() == n
        fa, fs = str(tmp_path / "whole.ply"), str(tmp_path / "slabs.ply")
        nv, nf = C.c_uint32(), C.c_uint32()
        ok, nva, nfa = app.save_mesh(fa)
        assert ok and sl.hkf_slabs_save_mesh(fs.encode(), C.byref(nv), C.byref(nf)) == 1
        assert (nv.value, nf.value) == (nva, nfa) and nfa > 1000
        assert open(fa, "rb").read() == open(fs, "rb").read()
    finally:
        sl.hkf_slabs_shutdown()
        app.close()
