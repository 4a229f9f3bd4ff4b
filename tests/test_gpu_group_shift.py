"""GPU: the moving volume on slab groups.  A group shifts its window by whole bricks on any axis -- brick layers travel between the members for a z
shift -- and every member's stored layers, halo included, are bit for bit what a whole-volume context holds there after kf_shift_volume; so are the
pose, the origin, the observed-voxel counts, the model maps of the merged raycast, the frames that follow and the marching cubes.

Geometry of test_gpu_group.py: 192^3 @ 3.0 m (cell 2^-6 m: the expected pose is exact in numpy fp32, as test_gpu_shift.moved_pose states it), VGA
camera, stock parameters, LOCAL backend, Scene S.  Every comparison is on bits."""
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
from hybkinectfu_amd import scene as S

from test_gpu_group import bits, check_frame, check_volume, whole_frame
from test_gpu_shift import moved_pose, np_shift, walk_pose, H_RES, H_SIZE, H_DIST
from test_gpu_shift import CAM as SMALL_CAM
import test_gpu_shift as SH

pytestmark = pytest.mark.gpu
P = S.STOCK
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RES, SIZE = 192, 3.0
CELL = SIZE / RES
CAM = S.vga_camera()
FUSED = 3
ERR_ARG, ERR_STATE = 1001, 1002


@pytest.fixture(autouse=True)
def _close_leaked():
    yield
    for g in G.live_groups():
        g.close()
    for c in K.live_contexts():
        c.close()


_FRAMES = {}


def frame(k):
    if k not in _FRAMES:
        _FRAMES[k] = S.render_depth_mm(S.trajectory_pose(k, SIZE), CAM, SIZE)
    return _FRAMES[k]


def new_whole(**kw):
    ctx = K.Context(K.camera(*CAM), RES, SIZE, P["volume_max_weight"], levels=3, **kw)
    ctx.set_pose(S.pose0(SIZE))
    return ctx


def fused_pair(cuts, n=FUSED, **kw):
    """a whole-volume context and a LOCAL group after the same n frames"""
    whole = new_whole(**kw)
    g = G.Group.local(K.camera(*CAM), RES, SIZE, cuts, **kw)
    for k in range(n):
        whole_frame(whole, frame(k), k)
        g.frame(frame(k), k)
    return whole, g


def pose_of(ctx):
    return ctx.track_result()[1]


def assert_members_hold(g, t, w, what):
    """every member's full stored range, halo included, equals the planes (t, w) of the whole volume"""
    for i, m in enumerate(g.members()):
        z0, z1 = m.stored
        mt, mw = m.download_volume(z0, z1)
        assert np.array_equal(bits(mt), bits(t[z0:z1])), (what, i, "tsdf")
        assert np.array_equal(bits(mw), bits(w[z0:z1])), (what, i, "weight")


def assert_same_maps(g, whole):
    for i, m in enumerate(g.members()):
        for level in range(3):
            for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                assert np.array_equal(bits(m.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (i, level, map_id)


def whole_raycast(ctx):
    ctx.raycast(None, P["raycast_increment_factor"] * P["integrate_sdf_trunc"], P["depth_trunc_min"], P["depth_trunc_max"])


# ---- 1. kf_shift_slab on a whole-volume context is kf_shift_volume -----------------------------------------------------------------------------
def test_shift_slab_on_a_whole_volume_context_equals_shift_volume():
    a, b = new_whole(), new_whole()
    for k in range(FUSED):
        whole_frame(a, frame(k), k)
        whole_frame(b, frame(k), k)
    assert a.slab_shift_needs(24) == (0, 0) and a.slab_layer_bytes() == (RES // 8) ** 2 * (4096 + 8)
    for d in ((8, 0, 0), (0, -16, 8), (0, 0, -24)):
        a.shift_volume(*d)
        b.shift_slab(*d)
        ta, wa = a.download_volume()
        tb, wb = b.download_volume()
        assert np.array_equal(bits(ta), bits(tb)) and np.array_equal(bits(wa), bits(wb)), d
        assert np.count_nonzero(wa) > 100000
        assert np.array_equal(bits(pose_of(a)), bits(pose_of(b))) and a.volume_origin() == b.volume_origin(), d
        assert a.stats()["weight_gt0"] == b.stats()["weight_gt0"] == np.count_nonzero(wa > 0), d
        whole_raycast(a)
        whole_raycast(b)
        for c in (a, b):
            c.downsample(True)
        for level in range(3):
            for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                assert np.array_equal(bits(a.download_map(map_id, level)), bits(b.download_map(map_id, level))), (d, level, map_id)
    assert a.volume_origin() == (8, -16, -16)
    a.close(); b.close()


def test_shift_slab_equals_shift_volume_with_colour_on_every_walked_axis():
    """The two launch forms of the one brick move, on whole-volume colour contexts (64^3: 8 bricks per axis) after five fused frames: each of x, y and z
    as the walked axis in both signs, a combined shift, and one that makes everything leave (|s| >= nb).  Bytes of tsdf, weight, colour, pose and origin,
    and of the model maps and the raycast colours after a raycast."""
    a, b = SH.make_ctx(64, True), SH.make_ctx(64, True)
    SH.fuse(a, range(5), True)
    SH.fuse(b, range(5), True)
    shifts = [(8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -8), (8, -8, 16), (0, -64, 0)]
    for d in shifts:
        a.shift_volume(*d)
        b.shift_slab(*d)
        pa, pb = SH.planes(a, True), SH.planes(b, True)
        for x, y, what in zip(pa, pb, ("tsdf", "weight", "colour")):
            assert SH.same_bits(x, y), (d, what)
        assert SH.same_bits(pose_of(a), pose_of(b)) and a.volume_origin() == b.volume_origin(), d
        if d != shifts[-1]:
            assert np.count_nonzero(pa[1]) > 1000 and np.any(pa[0] < 0) and np.count_nonzero(pa[2]) > 1000, d      # something moved
        else:
            assert not pa[1].any() and not pa[2].any()
        SH.raycast(a, True)
        SH.raycast(b, True)
        SH.assert_same_model(a, b, True)
    assert a.volume_origin() == (8, -72, 16)
    a.close(); b.close()


# ---- 2. a group shift equals the whole-volume shift --------------------------------------------------------------------------------------------
UNEVEN2, EVEN3 = [0, 40, 192], [0, 64, 128, 192]
SHIFTS = [(8, 0, 0), (0, -16, 0), (0, 0, 8), (0, 0, -8), (0, 0, 24), (0, 0, 48), (0, 0, -48), (16, -8, 24), (0, 0, 192), (0, 0, 0)]
CASES = [(c, d) for c in (UNEVEN2, EVEN3) for d in SHIFTS] + [(EVEN3, (0, 0, 72))]


@pytest.mark.parametrize("cuts,d", CASES, ids=["%d-%d_%d_%d" % ((len(c) - 1,) + d) for c, d in CASES])
def test_group_shift_equals_whole_volume_shift(cuts, d):
    whole, g = fused_pair(cuts)
    t0, w0 = whole.download_volume()
    assert np.count_nonzero(w0) > 100000 and np.any(t0 < 0)
    assert_members_hold(g, t0, w0, "before")                       # the precondition the local-if-stored rule rests on
    pose = pose_of(whole)
    calls = [m.raycast_form()["calls"] for m in g.members()]
    g.shift_volume(*d)
    whole.shift_volume(*d)
    if d == (0, 0, 0):
        assert [m.raycast_form()["calls"] for m in g.members()] == calls
    t1, w1 = np_shift(t0, d), np_shift(w0, d)
    assert_members_hold(g, t1, w1, "numpy")
    tw, ww = whole.download_volume()
    assert np.array_equal(bits(tw), bits(t1)) and np.array_equal(bits(ww), bits(w1))
    want = moved_pose(pose, d, CELL)
    for i, m in enumerate(g.members()):
        assert np.array_equal(bits(pose_of(m)), bits(want)), (i, pose_of(m), want)
        assert m.volume_origin() == whole.volume_origin() == d
    assert np.array_equal(bits(pose_of(whole)), bits(want))
    assert g.volume_origin() == d
    assert sum(m.stats()["weight_gt0"] for m in g.members()) == whole.stats()["weight_gt0"] == np.count_nonzero(w1 > 0)
    g.close(); whole.close()


# ---- 3. the stream goes on ---------------------------------------------------------------------------------------------------------------------
def test_the_stream_goes_on_after_a_group_shift():
    whole, g = fused_pair(EVEN3, max_triangles=600000)
    g.shift_volume(0, 0, 8)
    g.raycast()
    whole.shift_volume(0, 0, 8)
    whole_raycast(whole)
    whole.downsample(True)
    assert_same_maps(g, whole)
    assert int((whole.download_map(K.MAP_MODEL_VERTICES)[..., 3] != 0).sum()) > 10000
    for k in range(FUSED, FUSED + 2):
        whole_frame(whole, frame(k), k)
        g.frame(frame(k), k)
        check_frame(g, whole, k)
    check_volume(g, whole)
    thr = 300 * SIZE / RES
    whole.marching_cubes(thr)
    g.marching_cubes(thr)
    wt, gt = whole.triangles(), g.triangles()
    assert len(wt) > 1000 and gt.tobytes() == wt.tobytes()
    g.close(); whole.close()


# ---- 4. away and back --------------------------------------------------------------------------------------------------------------------------
def test_away_and_back():
    whole, g = fused_pair(UNEVEN2)
    t0, w0 = whole.download_volume()
    for d in ((0, 0, 16), (0, 0, -16)):
        g.shift_volume(*d)
        whole.shift_volume(*d)
    t1, w1 = whole.download_volume()
    assert np.array_equal(bits(t1[16:]), bits(t0[16:])) and np.array_equal(bits(w1[16:]), bits(w0[16:]))      # what never left the window
    assert not t1[:16].any() and not w1[:16].any()                # what left reads as never observed
    assert np.count_nonzero(w0[:16]) > 1000                       # ... and there was something to forget
    assert_members_hold(g, t1, w1, "back")
    assert g.volume_origin() == whole.volume_origin() == (0, 0, 0)
    assert np.array_equal(bits(pose_of(g.members()[0])), bits(pose_of(whole)))
    g.close(); whole.close()


# ---- 5. a colour group -------------------------------------------------------------------------------------------------------------------------
def test_colour_group_shift_carries_the_colour_planes():
    kcam = K.camera(*CAM)
    cuts = [0, 96, 192]
    whole = K.Context(kcam, RES, SIZE, P["volume_max_weight"], levels=3, has_color=True)
    whole.set_pose(S.pose0(SIZE))
    g = G.Group.local(kcam, RES, SIZE, cuts, has_color=True, angle_weight=True)
    rng = np.random.default_rng(11)
    inc = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]
    for k in range(FUSED):
        rgb = rng.integers(0, 256, (CAM[1], CAM[0], 3)).astype(np.uint8)
        whole.upload_depth_mm(frame(k)); whole.upload_rgb(rgb)
        whole.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
        whole.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
        whole.integrate(None, P["integrate_sdf_trunc"], P["integrate_depth_trunc"], has_color=True, angle_weight=True)
        whole.raycast(None, inc, P["depth_trunc_min"], P["depth_trunc_max"], has_color=True)
        g.frame(frame(k), k, rgb=rgb)
    t0, w0, c0 = whole.download_volume(color=True)
    assert np.count_nonzero(c0) > 100000
    for m in g.members():
        z0, z1 = m.stored
        mt, mw, mc = m.download_volume(z0, z1, color=True)
        assert np.array_equal(bits(mt), bits(t0[z0:z1])) and np.array_equal(bits(mw), bits(w0[z0:z1])) and np.array_equal(mc, c0[z0:z1])
    assert g.members()[0].slab_layer_bytes() == (RES // 8) ** 2 * (4096 + 2048 + 8)
    d = (0, 0, 24)
    pose = pose_of(whole)
    g.shift_volume(*d)
    whole.shift_volume(*d)
    t1, w1, c1 = np_shift(t0, d), np_shift(w0, d), np_shift(c0, d)
    tw, ww, cw = whole.download_volume(color=True)
    assert np.array_equal(bits(tw), bits(t1)) and np.array_equal(bits(ww), bits(w1)) and np.array_equal(cw, c1)
    for i, m in enumerate(g.members()):
        z0, z1 = m.stored
        mt, mw, mc = m.download_volume(z0, z1, color=True)
        assert np.array_equal(bits(mt), bits(t1[z0:z1])) and np.array_equal(bits(mw), bits(w1[z0:z1])), i
        assert np.array_equal(mc, c1[z0:z1]), i
        assert np.array_equal(bits(pose_of(m)), bits(moved_pose(pose, d, CELL))) and m.volume_origin() == d
    assert sum(m.stats()["weight_gt0"] for m in g.members()) == whole.stats()["weight_gt0"] == np.count_nonzero(w1 > 0)
    g.raycast()
    whole.raycast(None, inc, P["depth_trunc_min"], P["depth_trunc_max"], has_color=True)
    whole.downsample(True)
    assert_same_maps(g, whole)
    wrgb = whole.download_map(K.MAP_RAYCAST_RGB)
    assert wrgb.any()
    for m in g.members():
        assert np.array_equal(m.download_map(K.MAP_RAYCAST_RGB), wrgb)
    g.close(); whole.close()


# ---- 6. refusals touch nothing -----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    whole, g = fused_pair(UNEVEN2)
    t0, w0 = whole.download_volume()
    pose = pose_of(whole)
    calls = [(m.raycast_form()["calls"], m.fusion_form()["calls"]) for m in g.members()]
    with pytest.raises(G.GroupError) as e:
        g.shift_volume(4, 0, 0)
    assert e.value.status == G.ERR_ARG
    m0, m1 = g.members()
    lib = K.load()
    feed = torch.zeros(2 * m0.slab_layer_bytes(), dtype=torch.uint8, device="cuda")
    assert m0.slab_shift_needs(8) == (6, 7) and m1.slab_shift_needs(-8) == (3, 4) and m1.slab_shift_needs(8) == (0, 0)
    assert lib.kf_shift_slab(m0.h, 0, 0, 8, C.c_void_p(feed.data_ptr()), 6, 8) == ERR_ARG       # a feed range that is not the need
    assert lib.kf_shift_slab(m0.h, 0, 0, 8, C.c_void_p(feed.data_ptr()), 5, 6) == ERR_ARG
    assert lib.kf_shift_slab(m0.h, 0, 0, 8, None, 6, 7) == ERR_ARG                              # a need and no feed
    assert lib.kf_shift_slab(m0.h, 0, 0, 8, None, 0, 0) == ERR_ARG
    assert lib.kf_shift_slab(m1.h, 0, 0, 8, C.c_void_p(feed.data_ptr()), 6, 7) == ERR_ARG       # no need and a feed range
    assert lib.kf_shift_slab(m0.h, 0, 3, 0, None, 0, 0) == ERR_ARG
    assert lib.kf_slab_pack_layers(m0.h, 5, 7, C.c_void_p(feed.data_ptr())) == ERR_ARG          # member 0 stores brick layers [0, 6)
    assert lib.kf_slab_pack_layers(m0.h, 3, 3, C.c_void_p(feed.data_ptr())) == ERR_ARG
    assert_members_hold(g, t0, w0, "refused")
    for m in g.members():
        assert np.array_equal(bits(pose_of(m)), bits(pose)) and m.volume_origin() == (0, 0, 0)
    assert g.volume_origin() == (0, 0, 0)
    assert [(m.raycast_form()["calls"], m.fusion_form()["calls"]) for m in g.members()] == calls
    whole_frame(whole, frame(FUSED), FUSED)
    g.frame(frame(FUSED), FUSED)                                   # the group stayed usable
    check_frame(g, whole, FUSED)
    check_volume(g, whole)
    # a brick store or stream-out: whole-volume features of kf_shift_volume
    whole.brick_store_reserve(64)
    tw, ww = whole.download_volume()
    assert lib.kf_shift_slab(whole.h, 8, 0, 0, None, 0, 0) == ERR_STATE
    t2, w2 = whole.download_volume()
    assert np.array_equal(bits(t2), bits(tw)) and np.array_equal(bits(w2), bits(ww)) and whole.volume_origin() == (0, 0, 0)
    whole.brick_store_reserve(0)
    assert lib.kf_shift_slab(whole.h, 8, 0, 0, None, 0, 0) == 0
    g.close(); whole.close()


# ---- 7. RCCL -----------------------------------------------------------------------------------------------------------------------------------
def _child(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k == "KF_STATS_CROSSCHECK"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_shift_rccl_child.py"), mode], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "group shift rccl ok" in r.stdout, "child %s exited with %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_rccl_all_world1_shift_equals_plain_context():
    _child("all1")


def test_rccl_rank_world1_shift_equals_plain_context():
    _child("rank1")


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason="needs two or more visible devices")
def test_rccl_all_shift_over_every_visible_device():
    _child("alldev")


# ---- 8. the host class -------------------------------------------------------------------------------------------------------------------------
def test_slab_class_explicit_shift_equals_hybkinectfu(tmp_path):
    """HybKinectfuSlabs (LOCAL, 2 members) against HybKinectfu: a shift between frames, pose bits after every step, origins, the saved .ply"""
    app = H.App(RES, SIZE, CAM, max_triangles=600000)
    sl = H.SlabsApp(RES, SIZE, CAM, [0, 96, 192], max_triangles=600000)
    try:
        def same_pose(what):
            (oa, pa), (os_, ps) = app.pose(), sl.pose()
            assert oa and os_ and np.array_equal(bits(pa), bits(ps)), what
            return pa
        for k in range(3):
            assert app.process_frame(frame(k), k) and sl.process_frame(frame(k), k)
            same_pose(k)
        before = same_pose("before")
        assert not app.shift_volume(4, 0, 0) and not sl.shift_volume(4, 0, 0)
        assert app.volume_origin() == sl.volume_origin() == (0, 0, 0)
        assert app.shift_volume(8, -8, 16) and sl.shift_volume(8, -8, 16)
        assert app.volume_origin() == sl.volume_origin() == (8, -8, 16)
        assert np.array_equal(bits(same_pose("moved")), bits(moved_pose(before, (8, -8, 16), CELL)))
        for k in range(3, 6):
            assert app.process_frame(frame(k), k) and sl.process_frame(frame(k), k)
            same_pose(k)
        n = app.generate_mesh()
        assert n > 1000 and sl.generate_mesh() == n
        fa, fs = str(tmp_path / "whole.ply"), str(tmp_path / "slabs.ply")
        oka, nva, nfa = app.save_mesh(fa)
        oks, nvs, nfs = sl.save_mesh(fs)
        assert oka and oks and (nva, nfa) == (nvs, nfs) and nfa > 1000
        assert open(fa, "rb").read() == open(fs, "rb").read()
        v = H.app_mesh()["vertices"]                                # world coordinates: the scene sits where it sat in the first cube
        assert v[:, 2].min() > 0.2 * SIZE
    finally:
        sl.close()
        app.close()


def _walk(tmp_path, cls, name, dist, poses):
    path = str(tmp_path / name)
    trunc = 5 * H_SIZE / H_RES
    if cls == "app":
        app = H.App(H_RES, H_SIZE, SMALL_CAM, sdf_trunc=trunc, integrate_dist=3.6, traj_write=path)
    else:
        app = H.SlabsApp(H_RES, H_SIZE, SMALL_CAM, [0, 64, 128], sdf_trunc=trunc, integrate_dist=3.6, traj_write=path)
    try:
        app.set_recentre(dist)
        tracked, origins, out_poses = [], [], []
        for k, mm in enumerate(poses):
            tracked.append(app.process_frame(mm, k, stamp=float(k)))
            origins.append(app.volume_origin())
            out_poses.append(app.pose()[1].copy())
    finally:
        app.close()
    return tracked, origins, out_poses, open(path, "rb").read().replace(name.encode(), b"FILE")


def test_slab_class_recentres_like_hybkinectfu(tmp_path):
    """the walking camera of test_gpu_shift.py through both classes: the same shifts at the same frames, the same trajectory file; and with the
    policy at 0 the slab class writes the bytes it writes with the policy on and nothing to shift for"""
    n = 20
    depth = [S.render_depth_mm(walk_pose(k, n), SMALL_CAM, H_SIZE) for k in range(n)]
    a = _walk(tmp_path, "app", "walk_app.txt", H_DIST, depth)
    s = _walk(tmp_path, "slabs", "walk_slabs.txt", H_DIST, depth)
    assert all(a[0]) and all(s[0])
    assert a[1] == s[1] and a[1][-1] != (0, 0, 0)                  # the same shifts at the same frames, at least one
    for k, (pa, ps) in enumerate(zip(a[2], s[2])):
        assert np.array_equal(bits(pa), bits(ps)), k
    assert a[3] == s[3] and a[3].count(b"\n") == n + 3
    still = [S.render_depth_mm(S.trajectory_pose(k, H_SIZE), SMALL_CAM, H_SIZE) for k in range(6)]
    off = _walk(tmp_path, "slabs", "off.txt", 0.0, still)
    on = _walk(tmp_path, "slabs", "on.txt", H_DIST, still)
    ref = _walk(tmp_path, "app", "ref.txt", 0.0, still)
    assert all(off[0]) and all(o == (0, 0, 0) for o in off[1] + on[1])
    assert off[3] == on[3] == ref[3]
    for pa, ps in zip(off[2], ref[2]):
        assert np.array_equal(bits(pa), bits(ps))
