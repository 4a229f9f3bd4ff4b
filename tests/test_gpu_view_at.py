"""GPU: viewer frames of the whole map.  kf_render_view_at renders a VIRTUAL window -- the window as kf_shift_volume would assemble it at another origin, the
brick store's bricks restored -- without moving anything.  Expectations always come from the path that existed before: shift the window there,
kf_render_view, shift back.  Everything is compared as bytes: the picture and the bits of the float4 maps.  Shapes, stream and helpers are those of
test_gpu_shift.py, test_gpu_brickstore.py and test_gpu_mapmesh.py: 64 voxels at 2.0 m and 72 at 2.25 m (nine bricks per axis: ragged tables), a 160 x 120
context camera, six fused frames of Scene S, colour with the VGA colour camera, a store of 1024 bricks.  View cameras: the context's own, 200 x 90 (no
multiple of the 32 x 16 ray tile either way) and test_gpu_view.py's BIG."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_brickstore as B
import test_gpu_mapmesh as M
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda", 0)
P = G.P
CASES = B.CASES                                                   # (64, False), (72, False), (64, True)
CAP = B.CAP
ODD = (200, 90, 99.5, 44.5, 150.0, 150.0)
BIG = (416, 304, 207.5, 151.5, 340.0, 340.0)                      # test_gpu_view.BIG
CAMS = (G.CAM, ODD, BIG)
ARG, STATE = 1001, 1002
u32 = B.u32
f32 = np.float32


def modes_of(color):
    return (K.VIEW_NORMALS, K.VIEW_SHADED, K.VIEW_COLOR) if color else (K.VIEW_NORMALS, K.VIEW_SHADED)


def inc_of(ctx):
    return 0.7 * 5 * ctx.size / ctx.res


def render(ctx, frame, mode, pose, cam):
    """one view -- kf_render_view_at of `frame`, or kf_render_view for frame None -- as (image, v, n); the maps start as NaN, so every pixel must be written"""
    dv = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
    dn = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
    args = (pose, K.camera(*cam), inc_of(ctx), P["depth_trunc_min"], P["depth_trunc_max"], dv.data_ptr(), dn.data_ptr())
    if frame is None:
        ctx.render_view(mode, *args)
    else:
        ctx.render_view_at(mode, frame, *args)
    img = ctx.read_view()
    assert ctx.view_size() == (cam[0], cam[1]) and img.shape == (cam[1], cam[0], 4)
    return img, dv.cpu().numpy(), dn.cpu().numpy()


def same_view(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(u32(a[1]), u32(b[1])) and np.array_equal(u32(a[2]), u32(b[2]))


def hits(view):
    return int((view[1][..., 3] == 1.0).sum())


def look_pose(ctx, k=3):
    """an explicit pose, other than the tracked one: the stream's pose of frame k"""
    return S.trajectory_pose(k, ctx.size).astype(f32)


def views_wanted(color):
    """(mode, camera, explicit pose?) of every comparison: every mode, every camera, an explicit pose and NULL"""
    out = []
    for cam in CAMS:
        for mode in modes_of(color):
            for explicit in (True, False):
                out.append((mode, cam, explicit))
    return out


# ---- 1. the same frame ---------------------------------------------------------------------------------------------------------------------------
def assert_same_frame(ctx, color, what):
    """frame origin == origin: the call IS kf_render_view, picture and maps"""
    o = ctx.volume_origin()
    best = 0
    for mode, cam, explicit in views_wanted(color):
        pose = look_pose(ctx) if explicit else None
        if explicit:                                              # the stream's poses are the first cube's: into the window's coordinates
            pose = G.moved_pose(pose, o, ctx.size / ctx.res)
        got = render(ctx, o, mode, pose, cam)
        want = render(ctx, None, mode, pose, cam)
        assert same_view(got, want), (what, mode, cam, explicit, hits(got), hits(want))
        best = max(best, hits(want))
    assert best > 1000, (what, best)


@pytest.mark.parametrize("res,color", CASES)
def test_same_frame_is_render_view(res, color):
    ctx = M.fused(res, color)
    assert_same_frame(ctx, color, "store reserved, nothing in it")
    ctx.close()


@pytest.mark.parametrize("res,color", CASES)
def test_same_frame_without_a_store(res, color):
    """no store reserved is no error; the window stands away from the first cube"""
    ctx = M.fused(res, color, cap=0)
    ctx.shift_volume(8, -8, 16)
    assert_same_frame(ctx, color, "no store")
    ctx.close()


@pytest.mark.parametrize("res,color", CASES)
def test_window_takes_precedence_over_a_stale_store_copy(res, color):
    ctx = M.fused(res, color)
    ctx.shift_volume(32, 0, 0)
    ctx.shift_volume(-32, 0, 0)                                   # the store now holds copies of bricks that are back in the window
    G.raycast(ctx, color)
    for k in (6, 7):
        ok, _ = G.run_frame(ctx, k, color)
        assert ok, k
    # the case proves something only if a brick with a negative voxel differs between the window and its copy in the store
    t, _, _ = G.planes(ctx, color)
    keys, st, _, _ = ctx.brick_store(color=False)
    tb = B.bricks(t)
    nb = res // 8
    differ = 0
    for i, (x, y, z) in enumerate(keys.tolist()):
        if 0 <= x < nb and 0 <= y < nb and 0 <= z < nb:
            w = tb[z, y, x]
            differ += bool(np.any(w < 0) and not np.array_equal(u32(w), u32(st[i])))
    print(res, color, "bricks with a negative voxel whose store copy is stale:", differ)
    assert differ >= 1
    assert_same_frame(ctx, color, "stale copies in the store")
    ctx.close()


# ---- 2. elsewhere -------------------------------------------------------------------------------------------------------------------------------
ELSEWHERE = M.ELSEWHERE                                           # (32, 0, 0), (24, -24, 16), (0, 0, -24)


def store_only_bricks(ctx, frame):
    """[bz, by, bx] over the bricks of the virtual window at `frame`: the brick has a copy in the store and none in the window
    (test_gpu_mapmesh.store_only_cells' brick rule)"""
    nb = ctx.res // 8
    o = np.array(ctx.volume_origin()) // 8
    f = np.array(frame) // 8
    held = {tuple(k) for k in ctx.brick_store()[0].tolist()}
    only = np.zeros((nb, nb, nb), bool)
    for bz in range(nb):
        for by in range(nb):
            for bx in range(nb):
                w = f + (bx, by, bz)
                in_window = bool(np.all(w - o >= 0) and np.all(w - o < nb))
                only[bz, by, bx] = (tuple(int(v) for v in w) in held) and not in_window
    return only


def hits_in(view, only, cell):
    """hit pixels of a view whose vertex lies in a brick of the mask"""
    v = view[1]
    hit = v[..., 3] == 1.0
    b = np.floor(v[..., :3].astype(np.float64) / cell).astype(np.int64) // 8
    nb = only.shape[0]
    inside = hit & np.all((b >= 0) & (b < nb), axis=-1)
    b = np.clip(b, 0, nb - 1)
    return int((inside & only[b[..., 2], b[..., 1], b[..., 0]]).sum())


def by_shifting(ctx, frame, calls):
    """the expectation: the window moved to `frame`, kf_render_view with the same arguments, the window moved back"""
    o = ctx.volume_origin()
    d = tuple(int(f - x) for f, x in zip(frame, o))
    ctx.shift_volume(*d)
    assert ctx.volume_origin() == tuple(frame)
    out = [render(ctx, None, mode, pose, cam) for mode, pose, cam in calls]
    ctx.shift_volume(*[-x for x in d])
    return out


@pytest.mark.parametrize("d", ELSEWHERE)
@pytest.mark.parametrize("res,color", CASES)
def test_elsewhere_equals_shifting_there(res, color, d):
    """After shift_volume(d): the old place, d itself, half-way, and a far frame where nothing is resolved.  `got` is taken first, then the same context is
    shifted to the frame, rendered with kf_render_view and shifted back; with an explicit pose and with pose = NULL on both sides (the pose arithmetic).
    For the old-place frame and the context camera at least 100 hit pixels of the EXPECTATION have their vertex in a brick that only the store holds."""
    ctx = M.fused(res, color)
    ctx.shift_volume(*d)
    cell = ctx.size / res
    for frame in [(0, 0, 0), d, M.half(d), (1024, 0, 0)]:
        only = store_only_bricks(ctx, frame)                      # (every expectation below leaves more bricks in the store)
        explicit = G.moved_pose(look_pose(ctx), frame, cell)      # the stream's pose in the frame's coordinates
        calls = [(mode, pose, G.CAM) for mode in modes_of(color) for pose in (None, explicit)]
        calls += [(K.VIEW_SHADED, None, ODD), (modes_of(color)[-1], explicit, BIG)]
        got = [render(ctx, frame, mode, pose, cam) for mode, pose, cam in calls]
        want = by_shifting(ctx, frame, calls)
        for c, g, w in zip(calls, got, want):
            assert same_view(g, w), (frame, c[0], c[2], c[1] is None, hits(g), hits(w))
        if frame == (0, 0, 0):
            n_store = hits_in(want[0], only, cell)                # context camera, pose = NULL: the tracking pose looks at the old place
            print(res, color, d, "hit pixels with the vertex in a store-only brick:", n_store, "of", hits(want[0]))
            assert n_store >= 100, (d, n_store)
        if frame == (1024, 0, 0):
            assert not only.any()
            for g in got:
                assert hits(g) == 0 and not g[0][..., 3].any()
    ctx.close()


# ---- 3. a bystander ------------------------------------------------------------------------------------------------------------------------------
def state_of(ctx, color):
    out = {}
    t, w, c = G.planes(ctx, color)
    out["tsdf"], out["weight"] = u32(t).copy(), u32(w).copy()
    if color:
        out["color"] = c.copy()
    k, st, sw, sc = B.store_sorted(ctx)
    out["store_keys"], out["store_t"], out["store_w"] = k.copy(), u32(st).copy(), u32(sw).copy()
    if color:
        out["store_c"] = sc.copy()
    out["pose"] = u32(G.pose_of(ctx)).copy()
    for lv in range(3):
        out["v%d" % lv] = u32(ctx.download_map(K.MAP_MODEL_VERTICES, lv)).copy()
        out["n%d" % lv] = u32(ctx.download_map(K.MAP_MODEL_NORMALS, lv)).copy()
    if color:
        out["rgb"] = ctx.download_map(K.MAP_RAYCAST_RGB).copy()
    out["tris"] = np.ascontiguousarray(ctx.triangles()).view(np.uint8).copy()
    out["origin"] = np.array(ctx.volume_origin())
    out["store_count"] = np.array(ctx.brick_store_count(), np.uint64)
    s = ctx.stats(observed=False)                                 # (the counters only: asking for the observed voxels changes the count's bookkeeping)
    out["stats"] = np.array([s[k] for k in sorted(s)], np.uint64)
    return out, ctx.raycast_form()


def extractions(ctx, color):
    """what the four extraction calls give: whole volume, a region, a box of the old place, the map"""
    thr, res = M.thr_of(ctx), ctx.res
    out = []
    ctx.clear_triangles()
    ctx.marching_cubes(thr, has_color=color)
    out.append(M.take(ctx))
    ctx.marching_cubes_region(thr, (3, 9, 17), (41, 30, 55), has_color=color)
    out.append(M.take(ctx))
    out.append(M.at(ctx, (0, 0, 0), (0, 0, 0), (res, res, res), color, K.MC_WORLD)[0])
    ctx.marching_cubes_map(thr, has_color=color)
    out.append(M.take(ctx))
    return out


@pytest.mark.parametrize("res,color", CASES)
def test_a_view_elsewhere_is_a_bystander(res, color):
    ctxs = []
    for with_view in (True, False):                               # the second: a twin that never makes the call
        ctx = G.make_ctx(res, color, M.MAX_TRIS)
        ctx.brick_store_reserve(CAP)
        G.fuse(ctx, range(6), color)
        ctx.shift_volume(32, 0, 0)
        G.raycast(ctx, color)
        ctx.marching_cubes(M.thr_of(ctx), has_color=color)        # something in the triangle buffer
        ctxs.append(ctx)
    ctx, twin = ctxs
    cell = ctx.size / res
    explicit = G.moved_pose(look_pose(ctx), (0, 0, 0), cell)
    before, form_before = state_of(ctx, color)
    assert len(before["tris"]) > 0 and before["store_count"][0] > 0
    for mode in modes_of(color):
        for pose, cam in ((None, G.CAM), (explicit, ODD)):
            view = render(ctx, (0, 0, 0), mode, pose, cam)
            assert hits(view) > 500
            after, form_after = state_of(ctx, color)
            assert form_after == form_before, (form_before, form_after)
            for k in before:
                assert np.array_equal(before[k], after[k]), (mode, k)
    # the extraction calls give the bytes they gave before the call ...
    ctx.clear_triangles()
    ex_before = extractions(ctx, color)
    assert len(ex_before[0]) > 1000 and len(ex_before[2]) > 1000
    img1 = render(ctx, (0, 0, 0), K.VIEW_SHADED, None, G.CAM)
    ex_after = extractions(ctx, color)
    for a, b in zip(ex_before, ex_after):
        assert G.same_bits(a, b), (len(a), len(b))
    # ... and the other way round: an extraction of a virtual window between two views changes no picture
    img2 = render(ctx, (0, 0, 0), K.VIEW_SHADED, None, G.CAM)
    M.at(ctx, (8, 0, -8), (3, 9, 17), (41, 30, 55), color)
    img3 = render(ctx, (0, 0, 0), K.VIEW_SHADED, None, G.CAM)
    assert same_view(img1, img2) and same_view(img2, img3)
    # going on: two further frames fused and tracked on this context and on the twin
    for k in (6, 7):
        oks = [G.run_frame(c, k, color) for c in (ctx, twin)]
        assert oks[0][0] and oks[1][0], k
        assert np.array_equal(u32(oks[0][1]), u32(oks[1][1])), k
        render(ctx, (0, 0, 0), K.VIEW_NORMALS, None, ODD)
    ta, wa, ca = G.planes(ctx, color)
    tb, wb, cb = G.planes(twin, color)
    assert np.array_equal(u32(ta), u32(tb)) and np.array_equal(u32(wa), u32(wb))
    if color:
        assert np.array_equal(ca, cb)
    for c in ctxs:
        c.close()


# ---- 4. the raycast's switches --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def digest(env_extra):
    env = dict(os.environ)
    for k in ("KF_RAYCAST_SHARED_GRAD", "KF_RAYCAST_VIEW_HALF", "KF_RAYCAST_BOUNDS", "KF_RAYCAST_MESO", "KF_RAYCAST_NEG_LDS", "KF_RAYCAST_BOUNDS_MESO"):
        env.pop(k, None)
    env.update(dict(env_extra))
    env["PYTHONPATH"] = os.path.dirname(HERE) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(HERE, "view_at_digest.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("env", [(("KF_RAYCAST_NEG_LDS", "0"),), (("KF_RAYCAST_MESO", "0"),), (("KF_RAYCAST_BOUNDS", "0"),), (("KF_RAYCAST_BOUNDS", "2"),)])
def test_switches_give_the_same_view(env):
    """(32, 0, 0) / frame (0, 0, 0) in a process per setting (the switches are cached per process): the has-negative bits read from the virtual table in
    global memory, no meso table in LDS, no tile bounds, tile bounds through the super-cell list -- every digest equals the default run's"""
    ref = digest(())
    assert ref["hits"] > 1000, ref
    assert digest(env) == ref, env


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    ctx = M.fused(64, False)
    ctx.shift_volume(32, 0, 0)
    cam, inc, near, far = K.camera(*G.CAM), inc_of(ctx), P["depth_trunc_min"], P["depth_trunc_max"]
    pose = look_pose(ctx)
    with pytest.raises(K.KfError, match=str(STATE)):
        ctx.view_size()                                           # before any view
    ctx.render_view_at(K.VIEW_SHADED, (0, 0, 0), None, K.camera(*ODD), inc, near, far)
    size, img = ctx.view_size(), ctx.read_view()
    assert size == (ODD[0], ODD[1]) and int((img[..., 3] == 255).sum()) > 500
    state, form = state_of(ctx, False)

    def refused(code, mode, frame, cam_, inc_, c=ctx):
        with pytest.raises(K.KfError, match=str(code)):
            c.render_view_at(mode, frame, pose, cam_, inc_, near, far)
        if c is ctx:
            assert ctx.view_size() == size and np.array_equal(ctx.read_view(), img), (mode, frame)

    refused(ARG, K.VIEW_SHADED, None, cam, inc)                   # NULL frame, camera, increment
    refused(ARG, K.VIEW_SHADED, (0, 0, 0), None, inc)
    refused(ARG, K.VIEW_SHADED, (0, 0, 0), cam, None)
    for mode in (-1, 3):
        refused(ARG, mode, (0, 0, 0), cam, inc)
    for bad in ((0, 120), (160, 0), (4097, 120), (160, 4097)):
        refused(ARG, K.VIEW_NORMALS, (0, 0, 0), K.camera(bad[0], bad[1], *G.CAM[2:]), inc)
    refused(ARG, K.VIEW_NORMALS, (0, 0, 0), K.camera(160, 120, 79.5, 59.5, 0.0, 131.25), inc)
    refused(ARG, K.VIEW_NORMALS, (0, 0, 0), K.camera(160, 120, float("nan"), 59.5, 131.25, 131.25), inc)
    for frame in ((4, 0, 0), (0, -8, 3), (0, 12, 0)):             # no multiple of 8
        refused(ARG, K.VIEW_NORMALS, frame, cam, inc)
    refused(ARG, K.VIEW_NORMALS, (8 * (1 << 20) - 8 * (64 // 8) + 8, 0, 0), cam, inc)      # the frame's last brick would be 2^20
    refused(ARG, K.VIEW_NORMALS, (0, 0, -8 * (1 << 20) - 8), cam, inc)
    refused(STATE, K.VIEW_COLOR, (0, 0, 0), cam, inc)             # no colour plane
    lib = K.load()
    f = (C.c_int32 * 3)(0, 0, 0)
    rp = K.RaycastParams(inc)
    assert lib.kf_render_view_at(None, K.VIEW_SHADED, f, None, C.byref(cam), C.byref(rp), C.c_float(near), C.c_float(far), None, None) == ARG
    after, form_after = state_of(ctx, False)
    assert form_after == form
    for k in state:
        assert np.array_equal(state[k], after[k]), k
    # the last frame in range on either side is accepted: nothing there, no hit
    ctx.render_view_at(K.VIEW_NORMALS, (8 * (1 << 20) - 8 * (64 // 8), 0, -8 * (1 << 20)), pose, cam, inc, near, far)
    assert ctx.view_size() == (G.CAM[0], G.CAM[1]) and not ctx.read_view()[..., 3].any()
    slab = K.Context(K.camera(*G.CAM), 64, 2.0, P["volume_max_weight"], levels=3, slab=(0, 32), halo=8)
    refused(STATE, K.VIEW_NORMALS, (0, 0, 0), cam, inc, slab)     # a z-slab context
    with pytest.raises(K.KfError, match=str(STATE)):
        slab.view_size()
    slab.close()
    ctx.close()


# ---- 6. the host classes ---------------------------------------------------------------------------------------------------------------------------
def test_host_classes_return_the_contexts_bytes():
    res, size, cam = 64, 2.0, G.CAM
    trunc = 5 * size / res
    app = H.App(res, size, cam, sdf_trunc=trunc, integrate_dist=G.GATE)
    app.set_brick_store(CAP)
    for k in range(4):
        assert app.process_frame(G.frame(k, size), k)
    assert app.shift_volume(32, 0, 0)
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), res, size)
    assert ctx.brick_store_count()[0] > 0
    inc = float(f32(0.7) * f32(trunc))                           # hkf_app_init: 0.7f * sdf_trunc
    near, far = P["depth_trunc_min"], P["depth_trunc_max"]
    cell = size / res
    explicit = look_pose(ctx)
    for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
        for frame in ((0, 0, 0), (16, 0, -8)):
            for pose in (G.moved_pose(explicit, frame, cell), None):
                got = app.render_view_at(mode, frame, pose, ODD)
                ctx.render_view_at(mode, frame, pose, K.camera(*ODD), inc, near, far)
                exp = ctx.read_view()
                assert np.array_equal(got, exp) and int((got[..., 3] == 255).sum()) >= 400, (mode, frame)
        # a view of the map from a world pose: the frame hkf_view_frame chooses, the pose in its coordinates
        frames = []
        for world in (explicit, G.moved_pose(explicit, (-12, 4, 8), cell)):      # the second: 12 voxels to the right, 4 up, 8 back -- the box stays in sight
            frame, local = H.view_frame(world, size, res)
            frames.append(frame)
            got = app.render_map_view(mode, world, ODD)
            ctx.render_view_at(mode, frame, local, K.camera(*ODD), inc, near, far)
            exp = ctx.read_view()
            assert np.array_equal(got, exp) and int((got[..., 3] == 255).sum()) >= 400, (mode, frame)
        assert frames[0] != frames[1] and any(frames[1]), frames
    with pytest.raises(K.KfError):
        app.render_view_at(K.VIEW_COLOR, (0, 0, 0), explicit, ODD)           # the application has no colour plane
    with pytest.raises(K.KfError):
        app.render_view_at(K.VIEW_SHADED, (4, 0, 0), explicit, ODD)
    ctx.close()
    app.close()
