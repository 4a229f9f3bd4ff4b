"""GPU: the moving volume.  kf_shift_volume slides the TSDF window by whole bricks in place; everything is checked bit for bit against the
numpy slice-and-zero of the planes taken before, and against a fresh context that gets the shifted planes uploaded ("shifted here" equals
"uploaded there"): model maps at every pyramid level, marching cubes, and the frames that follow.

Volumes whose voxel size is a power of two (64 @ 2.0 m, 72 @ 2.25 m, 128 @ 4.0 m: cell = 1 / 32): (float)d * cell is exact and t - d * cell is one
correctly rounded subtraction, so numpy fp32 states the expected pose bit for bit.  72 gives 9 bricks per axis: macro, super and meso cells
and the last word of the per-brick bits are all ragged."""
import ctypes as C
import os

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = S.STOCK
CAM = (160, 120, 79.5, 59.5, 131.25, 131.25)
f32 = np.float32
SIZES = {64: 2.0, 72: 2.25}
GATE = 2.5                                                        # integration distance: the back wall of the box lies at 1.8 m / 1.99 m


RGB_CAM = S.vga_camera()          # the colour image: the fusion pass projects into it with the reference's hard-coded VGA intrinsics (integrateVolume.cu:54-63),
                                  # and a voxel whose projection misses the image is not fused at all -- a colour context needs the VGA colour camera


def bgr(k):
    y, x = np.mgrid[0:RGB_CAM[1], 0:RGB_CAM[0]]
    return np.stack([(x * 3 + k * 7) % 256, (y * 5 + x) % 256, (x + 2 * y + 31 * k) % 256], axis=-1).astype(np.uint8)


_FRAMES = {}


def frame(k, size):
    if (k, size) not in _FRAMES:
        _FRAMES[(k, size)] = S.render_depth_mm(S.trajectory_pose(k, size), CAM, size)
    return _FRAMES[(k, size)]


def make_ctx(res, color=False, max_triangles=0, **kw):
    if color:
        kw["rgb_cam"] = K.camera(*RGB_CAM)
    return K.Context(K.camera(*CAM), res, SIZES[res], P["volume_max_weight"], levels=3, max_triangles=max_triangles, has_color=color, **kw)


def run_frame(ctx, k, color=False, tracker="icp"):
    """one frame of the stream on the device-resident pose: preprocess, track, integrate, raycast; returns (tracked, pose)"""
    size = ctx.size
    trunc = 5 * size / ctx.res
    ctx.upload_depth_mm(frame(k, size))
    if color:
        ctx.upload_rgb(bgr(k))
    ctx.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
    if tracker == "sdf":
        ctx.sdf_track(k, P["sdf_max_iter_nums"], P["camera_shake_dist"], P["camera_shake_angle"])
    else:
        ctx.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
    ctx.integrate(None, trunc, GATE, has_color=color, angle_weight=color)
    raycast(ctx, color)
    ok, pose, _, _ = ctx.track_result()
    return ok, pose


def raycast(ctx, color=False):
    ctx.raycast(None, 0.7 * 5 * ctx.size / ctx.res, P["depth_trunc_min"], P["depth_trunc_max"], has_color=color)


def fuse(ctx, frames, color=False, tracker="icp"):
    ctx.set_pose(S.pose0(ctx.size))
    for k in frames:
        ok, _ = run_frame(ctx, k, color, tracker)
        assert ok or tracker == "sdf", k                          # (the SDF tracker may give a frame up; both sides of a comparison then do)


def planes(ctx, color=False):
    return ctx.download_volume(color=True) if color else ctx.download_volume() + (None,)


def np_shift(a, d):
    """out[z, y, x] = a[z + dz, y + dy, x + dx] inside the volume, zero elsewhere (a: planes in (z, y, x[, c]) order, d = (dx, dy, dz))"""
    out = np.zeros_like(a)
    R = a.shape[0]
    sl_dst, sl_src = [], []
    for s in (d[2], d[1], d[0]):
        if abs(s) >= R:
            return out
        sl_dst.append(slice(max(0, -s), R - max(0, s)))
        sl_src.append(slice(max(0, s), R - max(0, -s)))
    out[tuple(sl_dst)] = a[tuple(sl_src)]
    return out


def moved_pose(pose, d, cell):
    out = np.array(pose, f32)
    for i in range(3):
        out[i, 3] = f32(out[i, 3]) - f32(d[i]) * f32(cell)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def pose_of(ctx):
    return ctx.track_result()[1]


# ---- 1. the move itself --------------------------------------------------------------------------------------------------------------------
SHIFTS = [(8, 0, 0), (-8, 0, 0), (0, 16, 0), (0, -8, 0), (0, 0, 8), (0, 0, -24), (16, -8, 24), (0, 0, 0)]


@pytest.mark.parametrize("res,color", [(64, False), (72, False), (64, True)])
def test_shift_moves_planes_pose_and_origin(res, color):
    """every shift against the numpy slice-and-zero of the planes taken before it; the shifts accumulate, so does kf_volume_origin"""
    ctx = make_ctx(res, color)
    fuse(ctx, range(6), color)
    cell = ctx.size / res
    assert cell == 1.0 / 32
    t, w, c = planes(ctx, color)
    assert np.count_nonzero(w) > 1000 and np.any(t < 0)
    pose = pose_of(ctx)
    origin = np.zeros(3, np.int64)
    assert ctx.volume_origin() == (0, 0, 0)
    for d in SHIFTS + ([(64, 0, 0)] if res == 64 else []):        # the last one: everything leaves
        ctx.shift_volume(*d)
        t, w = np_shift(t, d), np_shift(w, d)
        c = np_shift(c, d) if color else None
        pose = moved_pose(pose, d, cell)
        origin += d
        gt, gw, gc = planes(ctx, color)
        assert np.array_equal(gt.view(np.uint32), t.view(np.uint32)), d       # as integers: -0.0 cannot hide
        assert np.array_equal(gw.view(np.uint32), w.view(np.uint32)), d
        if color:
            assert np.array_equal(gc, c), d
        assert ctx.volume_origin() == tuple(origin), d
        ok, got_pose, _, _ = ctx.track_result()
        assert ok and np.array_equal(got_pose.view(np.uint32), pose.view(np.uint32)), (d, got_pose, pose)
        assert ctx.stats()["weight_gt0"] == np.count_nonzero(w > 0), d         # re-based from the moved volume
    if res == 64:
        assert not np.any(w) and not np.any(t)
    ctx.reset_volume()
    assert ctx.volume_origin() == (0, 0, 0)
    ctx.close()


# ---- 2. + 3. derived state, and going on ---------------------------------------------------------------------------------------------------
def shifted_pair(res, d, color=False, defer=None, tracker="icp", max_triangles=0):
    """A: 6 frames fused, then shifted on the device.  B: a fresh context that gets the numpy-shifted planes and the translated pose.
    Both exist from the start, so both choose their launch forms with two contexts alive."""
    a = make_ctx(res, color, max_triangles)
    b = make_ctx(res, color, max_triangles)
    if defer is not None:
        a.set_defer(1 if defer else 0)
        b.set_defer(0)
    fuse(a, range(6), color, tracker)
    if defer:
        assert a.fusion_form()["defer"] == 1                      # the frames before the shift ran the deferred form
    t, w, c = planes(a, color)
    pose = pose_of(a)
    a.shift_volume(*d)
    b.upload_volume(np_shift(t, d), np_shift(w, d), np_shift(c, d) if color else None)
    b.set_pose(moved_pose(pose, d, a.size / res))
    raycast(a, color)
    raycast(b, color)
    return a, b


def assert_same_model(a, b, color):
    for ctx in (a, b):
        ctx.downsample(True)                                      # levels 1 and 2 from the level 0 just raycast, on both sides
    for level in range(3):
        for m in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
            assert same_bits(a.download_map(m, level), b.download_map(m, level)), (m, level)
    if color:
        assert same_bits(a.download_map(K.MAP_RAYCAST_RGB), b.download_map(K.MAP_RAYCAST_RGB))


@pytest.mark.parametrize("res,d,color", [(64, (16, -8, 8), False), (72, (8, -16, -8), False), (64, (-8, 8, 16), True)])
def test_shifted_equals_uploaded(res, d, color):
    """a stale skip table, a missed macro mark, a has-negative bit left behind or class tables not zeroed again would show here"""
    a, b = shifted_pair(res, d, color, max_triangles=300000)
    v0 = a.download_map(K.MAP_MODEL_VERTICES)
    assert np.count_nonzero(v0[..., 3]) > 2000                    # the raycast really sees the moved model
    assert_same_model(a, b, color)
    thr = 300 * a.size / res
    a.marching_cubes(thr, has_color=color)                        # A has extracted nothing before: its class tables start from the moved flags
    b.marching_cubes(thr, has_color=color)
    ta, tb = a.triangles(), b.triangles()
    assert len(ta) > 1000 and same_bits(ta, tb)
    # a second shift and a second extraction on A: the class tables of the first extraction must be zeroed again
    t, w, c = planes(a, color)
    d2 = (-d[0], 8, -8)
    a.shift_volume(*d2)
    b.upload_volume(np_shift(t, d2), np_shift(w, d2), np_shift(c, d2) if color else None)
    for ctx in (a, b):
        ctx.clear_triangles()
        ctx.marching_cubes(thr, has_color=color)
    assert same_bits(a.triangles(), b.triangles())
    a.close(); b.close()


@pytest.mark.parametrize("res,d,defer,tracker", [(64, (16, -8, 8), None, "icp"), (72, (8, -16, -8), None, "icp"), (64, (16, -8, 8), True, "icp"),
                                                 (72, (-8, 8, 8), True, "icp"), (64, (8, 8, -8), None, "sdf")])
def test_going_on_after_the_shift(res, d, defer, tracker):
    """the next 4 frames of the stream on A (shifted) and on B (uploaded): pose bits after every frame, the final planes"""
    a, b = shifted_pair(res, d, False, defer, tracker)
    for k in range(6, 10):
        oka, pa = run_frame(a, k, False, tracker)
        okb, pb = run_frame(b, k, False, tracker)
        assert oka == okb and (oka or tracker == "sdf"), k
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), (k, pa, pb)
        if defer:
            assert a.fusion_form()["defer"] == 1 and b.fusion_form()["defer"] == 0       # the words travelled with their bricks: deferral stays in force
    ta, wa, _ = planes(a)
    tb, wb, _ = planes(b)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(wa.view(np.uint32), wb.view(np.uint32))
    assert a.stats()["weight_gt0"] == np.count_nonzero(wa > 0)
    a.close(); b.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [False, True])
def test_refused_shift_touches_nothing(slab):
    res = 64
    ctx = make_ctx(res, slab=(0, 32), halo=8) if slab else make_ctx(res)
    fuse(ctx, range(1))
    t, w = ctx.download_volume()
    assert np.count_nonzero(w) > 1000
    pose, calls, n_obs = pose_of(ctx), ctx.raycast_form()["calls"], ctx.stats()["weight_gt0"]
    d = (8, 0, 0) if slab else (4, 0, 0)
    assert ctx.lib.kf_shift_volume(ctx.h, *d) == 1001             # KF_ERR_ARG
    if not slab:
        assert ctx.lib.kf_shift_volume(ctx.h, 8, 0, -3) == 1001
    else:
        assert ctx.lib.kf_shift_volume(ctx.h, 0, 0, 0) == 0       # no shift at all is no error anywhere
    t2, w2 = ctx.download_volume()
    assert np.array_equal(t2.view(np.uint32), t.view(np.uint32)) and np.array_equal(w2.view(np.uint32), w.view(np.uint32))
    assert np.array_equal(pose_of(ctx).view(np.uint32), pose.view(np.uint32))
    assert ctx.raycast_form()["calls"] == calls and ctx.volume_origin() == (0, 0, 0)
    assert ctx.stats()["weight_gt0"] == n_obs
    ctx.close()


# ---- 5. the host class ---------------------------------------------------------------------------------------------------------------------
H_RES, H_SIZE, H_DIST = 128, 4.0, 0.35                            # cell 1 / 32; the resting focus point lies 0.3 m in front of the centre


def walk_pose(k, n):
    """Scene S's 2 cm circle plus a translation of 0.5 m along x over n frames"""
    p = S.trajectory_pose(k, H_SIZE)
    p[0, 3] += 0.5 * k / (n - 1)
    return p


def read_traj(path):
    rows = [l.split() for l in open(path).read().splitlines() if l and not l.startswith("#")]
    return np.array([[float(x) for x in r] for r in rows])


def host_run(tmp_path, name, dist, poses):
    path = str(tmp_path / name)
    app = H.App(H_RES, H_SIZE, CAM, sdf_trunc=5 * H_SIZE / H_RES, integrate_dist=3.6, traj_write=path)
    app.set_recentre(dist)
    tracked, origins = [], []
    for k, p in enumerate(poses):
        tracked.append(app.process_frame(S.render_depth_mm(p, CAM, H_SIZE), k, stamp=float(k)))
        origins.append(app.volume_origin())
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*CAM), H_RES, H_SIZE)
    vol = ctx.download_volume()
    _, pose = app.pose()
    app.close()
    return tracked, origins, read_traj(path), open(path, "rb").read(), vol, pose


def test_host_class_recentres_on_a_walking_camera(tmp_path):
    """A real translated stream (rendered from Scene S with the camera walking 0.5 m along x over 20 frames), tracked by the host class with the
    policy on: at least one shift, every frame tracked, the recorded WORLD trajectory continuous across it."""
    n = 20
    poses = [walk_pose(k, n) for k in range(n)]
    tracked, origins, traj, _, _, pose = host_run(tmp_path, "walk.txt", H_DIST, poses)
    assert all(tracked)
    assert origins[0] == (0, 0, 0) and origins[-1] != (0, 0, 0) and all(o % 8 == 0 for o in origins[-1])
    assert len(traj) == n
    gt = np.stack([p[:3, 3] for p in poses])
    assert np.max(np.abs(traj[:, 1:4] - gt)) < 0.05                # world coordinates: a missing origin * cell would be a whole brick, 0.25 m
    assert np.max(np.abs(np.diff(traj[:, 1:4], axis=0))) < 0.05   # no jump where the window moved (a brick is 0.25 m)
    cell = H_SIZE / H_RES
    assert np.max(np.abs(pose[:3, 3] + np.array(origins[-1]) * cell - gt[-1])) < 0.05     # the pose itself lives in the window


def test_host_class_policy_off_changes_nothing(tmp_path):
    """Scene S's own 2 cm circle: with the policy on at 0.35 m nothing ever shifts, and trajectory file and volume equal, byte for byte, the run
    with fRecentreDist = 0 -- the path every existing run takes."""
    poses = [S.trajectory_pose(k, H_SIZE) for k in range(8)]
    off = host_run(tmp_path, "off.txt", 0.0, poses)
    on = host_run(tmp_path, "on.txt", H_DIST, poses)
    assert all(off[0]) and all(on[0])
    assert all(o == (0, 0, 0) for o in off[1] + on[1])
    assert off[3].replace(b"off.txt", b"on.txt") == on[3] and len(off[2]) == 8
    assert same_bits(off[4][0], on[4][0]) and same_bits(off[4][1], on[4][1])


def test_host_class_explicit_shift(tmp_path):
    """HybKinectfu::shiftVolume between frames of Scene S: tracking goes on, the saved mesh and the pose come out in world coordinates"""
    size, res = 2.0, 64
    app = H.App(res, size, CAM, sdf_trunc=5 * size / res, integrate_dist=GATE, max_triangles=300000)
    for k in range(4):
        assert app.process_frame(frame(k, size), k)
    _, before = app.pose()
    assert not app.shift_volume(4, 0, 0) and app.volume_origin() == (0, 0, 0)
    assert app.shift_volume(8, -8, 16) and app.volume_origin() == (8, -8, 16)
    _, after = app.pose()
    assert np.array_equal(after.view(np.uint32), moved_pose(before, (8, -8, 16), size / res).view(np.uint32))
    for k in range(4, 7):
        assert app.process_frame(frame(k, size), k)
    _, pose = app.pose()
    gt = S.trajectory_pose(6, size)[:3, 3]
    assert np.max(np.abs(pose[:3, 3] + np.array([8, -8, 16]) * (size / res) - gt)) < 0.01
    assert app.generate_mesh() > 1000
    ok, nv, nf = app.save_mesh(str(tmp_path / "moved.ply"))
    assert ok and nv > 500
    v = H.app_mesh()["vertices"]
    # the scene sits in [0.25, 0.75] * size of the FIRST cube: world coordinates, although the window has moved by (0.25, -0.25, 0.5) m
    assert v[:, 0].min() > 0.2 * size and v[:, 0].max() < 0.8 * size and v[:, 1].min() > 0.2 * size and v[:, 1].max() < 0.8 * size
    assert v[:, 2].min() > 0.2 * size and v[:, 2].max() < 0.8 * size + 5 * size / res
    app.close()
