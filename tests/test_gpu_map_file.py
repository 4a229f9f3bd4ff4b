"""GPU: saving and loading the whole map.  kf_write_brick_store is kf_read_brick_store's inverse; kf_brick_store_capture copies the window into the
store and is a bystander; kf_place_window leaves what capture + a shift far away + a shift to the target leave; HybKinectfu::saveMap / loadMap carry a
session across two applications.  Shapes, stream and helpers are those of test_gpu_shift.py and test_gpu_brickstore.py: 64 voxels at 2.0 m and 72 at
2.25 m (cell 1 / 32, so (float)d * cell is exact; 72 gives ragged tables), the 160 x 120 camera, 6 fused frames of Scene S, a store of 1024 bricks,
colour at 64.  Everything is compared as integers, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_brickstore as B
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
u32 = B.u32
CAP = B.CAP
CASES = B.CASES
ARG, STATE, ALLOC = 1001, 1002, 1003


def same_store(a, b):
    """two sorted read-outs (keys, tsdf, weight, colour) as bits"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(u32(a[1]), u32(b[1])) and np.array_equal(u32(a[2]), u32(b[2])) and
            ((a[3] is None and b[3] is None) or np.array_equal(a[3], b[3])))


def same_planes(a, b, color=False):
    pa, pb = G.planes(a, color), G.planes(b, color)
    return np.array_equal(u32(pa[0]), u32(pb[0])) and np.array_equal(u32(pa[1]), u32(pb[1])) and (not color or np.array_equal(pa[2], pb[2]))


def planes_bits(ctx, color=False):
    t, w, c = G.planes(ctx, color)
    return u32(t).copy(), u32(w).copy(), (c.copy() if color else None)


def equal_bits(p, q):
    return np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and (p[2] is None or np.array_equal(p[2], q[2]))


def write_raw(ctx, n, keys, t, w, c):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return ctx.lib.kf_write_brick_store(ctx.h, n, p(keys), p(t), p(w), p(c))


# ---- 1. write is read's inverse --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_write_is_reads_inverse(res, color):
    a = B.fused_ctx(res, color)
    a.shift_volume(32, 0, 0)
    keys, t, w, c = a.brick_store()
    n = len(keys)
    print(res, color, "bricks through the store", n)
    assert n >= 20 and a.brick_store_count() == (n, 0, 0)
    b = G.make_ctx(res, color)
    b.brick_store_reserve(CAP)
    order = np.random.default_rng(3).permutation(n)
    cut = (n // 2) | 1                                            # an odd index
    for part in (order[:cut], order[cut:]):
        b.write_brick_store(keys[part], t[part], w[part], c[part] if color else None)
    want = B.store_sorted(a)
    assert same_store(B.store_sorted(b), want) and b.brick_store_count() == a.brick_store_count()
    b.write_brick_store(keys, t, w, c)                            # the same entries again: found, overwritten with themselves
    assert same_store(B.store_sorted(b), want) and b.brick_store_count() == (n, 0, 0)
    t2, w2 = t.copy(), w.copy()                                   # a changed brick under a held key: overwritten in place
    t2[5] = -t2[5]; w2[5] = w2[5] + 1
    c2 = c.copy() if color else None
    if color:
        c2[5] = 255 - c2[5]
    b.write_brick_store(keys[5:6], t2[5:6], w2[5:6], c2[5:6] if color else None)
    o = np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))
    assert same_store(B.store_sorted(b), (keys[o], t2[o], w2[o], c2[o] if color else None)) and b.brick_store_count() == (n, 0, 0)
    fresh = np.array([[100, -100, 7]], np.int32)                  # no weight > 0: no slot
    b.write_brick_store(fresh, t[:1], np.zeros_like(w[:1]), c[:1] if color else None)
    assert b.brick_store_count() == (n, 0, 0) and not np.any(np.all(b.brick_store()[0] == fresh[0], axis=1))
    a.close(); b.close()


def test_written_colour_defaults_to_zero():
    a = B.fused_ctx(64, True)
    a.shift_volume(32, 0, 0)
    keys, t, w, c = a.brick_store()
    b = G.make_ctx(64, True)
    b.brick_store_reserve(CAP)
    b.write_brick_store(keys, t, w, None)
    got = B.store_sorted(b)
    assert np.array_equal(got[0], B.store_sorted(a)[0]) and not np.any(got[3])
    a.close(); b.close()


# ---- 2. a full store drops -----------------------------------------------------------------------------------------------------------------------
def test_a_full_store_drops():
    a = B.fused_ctx(64)
    a.shift_volume(32, 0, 0)
    keys, t, w, _ = a.brick_store()
    n = len(keys)
    assert n > 8
    b = G.make_ctx(64)
    b.brick_store_reserve(8)
    b.write_brick_store(keys, t, w)
    assert b.brick_store_count() == (8, n - 8, 0)
    gk, gt, gw, _ = b.brick_store()
    where = {tuple(k): i for i, k in enumerate(keys.tolist())}
    assert len({tuple(k) for k in gk.tolist()}) == 8              # every held key once: a dropped key is not among them, a look-up of it misses
    for i, k in enumerate(gk.tolist()):
        j = where[tuple(k)]
        assert np.array_equal(u32(gt[i]), u32(t[j])) and np.array_equal(u32(gw[i]), u32(w[j])), k
    b.place_window(0, 0, 0)                                       # every written key lies in the window at the origin: the held ones are found, the dropped ones miss
    assert b.brick_store_count() == (8, n - 8, 8)
    wb = B.bricks(G.planes(b)[1])
    assert sorted((x, y, z) for z in range(8) for y in range(8) for x in range(8) if np.any(wb[z, y, x] > 0)) == sorted(tuple(k) for k in gk.tolist())
    a.close(); b.close()


# ---- 3. refusals touch nothing ---------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    ctx = B.fused_ctx(64)
    ctx.shift_volume(32, 0, 0)
    keys, t, w, _ = ctx.brick_store()
    n = len(keys)
    store, planes, counts, origin, pose = B.store_sorted(ctx), planes_bits(ctx), ctx.brick_store_count(), ctx.volume_origin(), G.pose_of(ctx)
    t2, w2 = np.ascontiguousarray(t[:2] + 1), np.ascontiguousarray(w[:2] + 1)
    twice = np.ascontiguousarray(np.stack([keys[0], keys[0]]))
    assert write_raw(ctx, 2, twice, t2, w2, None) == ARG          # a key twice in one call
    for bad in ((1 << 20, 0, 0), (0, -(1 << 20) - 1, 0), (0, 0, 1 << 21)):
        far = np.ascontiguousarray(np.stack([keys[1], np.array(bad, np.int32)]))
        assert write_raw(ctx, 2, far, t2, w2, None) == ARG, bad
    k2 = np.ascontiguousarray(keys[:2])
    assert write_raw(ctx, 2, None, t2, w2, None) == ARG and write_raw(ctx, 2, k2, None, w2, None) == ARG and write_raw(ctx, 2, k2, t2, None, None) == ARG
    assert write_raw(ctx, 2, k2, t2, w2, np.zeros((2, 512, 3), np.uint8)) == STATE      # colour without a colour plane
    assert ctx.lib.kf_place_window(ctx.h, 4, 0, 0) == ARG and ctx.lib.kf_place_window(ctx.h, 8, -12, 0) == ARG
    assert ctx.lib.kf_place_window(ctx.h, 8 * (1 << 20), 0, 0) == ARG                   # the new window would leave the key range
    assert same_store(B.store_sorted(ctx), store) and equal_bits(planes_bits(ctx), planes) and ctx.brick_store_count() == counts
    assert ctx.volume_origin() == origin and np.array_equal(u32(G.pose_of(ctx)), u32(pose))
    ctx.close()
    bare = G.make_ctx(64)                                          # no store
    G.fuse(bare, range(2))
    planes = planes_bits(bare)
    assert write_raw(bare, 2, k2, t2, w2, None) == STATE and bare.lib.kf_brick_store_capture(bare.h) == STATE and bare.lib.kf_place_window(bare.h, 8, 0, 0) == STATE
    assert equal_bits(planes_bits(bare), planes) and bare.volume_origin() == (0, 0, 0) and bare.brick_store_count() == (0, 0, 0)
    bare.close()
    slab = G.make_ctx(64, slab=(0, 32), halo=8)                    # a z-slab context: the store stays a whole-volume feature
    assert slab.lib.kf_brick_store_capture(slab.h) == ARG and slab.lib.kf_place_window(slab.h, 8, 0, 0) == ARG
    assert write_raw(slab, 2, k2, t2, w2, None) == STATE
    slab.close()


# ---- 4. capture is a bystander and completes the store ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,defer", [(64, 1), (64, 0), (72, 1)])
def test_capture_is_a_bystander_and_completes_the_store(res, defer):
    a, b = G.make_ctx(res), G.make_ctx(res)
    for ctx in (a, b):
        ctx.set_defer(defer)
        ctx.brick_store_reserve(CAP)
        G.fuse(ctx, range(6))
        assert ctx.fusion_form()["defer"] == defer
    a.brick_store_capture()
    assert np.array_equal(u32(G.pose_of(a)), u32(G.pose_of(b))) and same_planes(a, b) and a.volume_origin() == (0, 0, 0)
    # the store alone is the whole map: the numpy brick model of the downloaded planes, the weights being the true weights
    t, w, _ = G.planes(a)
    tb, wb = B.bricks(t), B.bricks(w)
    nb = res // 8
    model = {(x, y, z): (tb[z, y, x], wb[z, y, x]) for z in range(nb) for y in range(nb) for x in range(nb) if np.any(wb[z, y, x] > 0)}
    print(res, defer, "observed bricks", len(model))
    assert len(model) >= 100 and a.brick_store_count() == (len(model), 0, 0) and b.brick_store_count() == (0, 0, 0)
    gk, gt, gw, _ = B.store_sorted(a)
    mk = sorted(model, key=lambda k: (k[2], k[1], k[0]))
    assert np.array_equal(gk, np.array(mk, np.int32))
    assert np.array_equal(u32(gt), u32(np.stack([model[k][0] for k in mk]))) and np.array_equal(u32(gw), u32(np.stack([model[k][1] for k in mk])))
    for k in range(6, 10):
        oka, pa = G.run_frame(a, k)
        okb, pb = G.run_frame(b, k)
        assert oka and okb and np.array_equal(u32(pa), u32(pb)), (k, pa, pb)
        assert same_planes(a, b), k
        assert a.fusion_form()["defer"] == defer and b.fusion_form()["defer"] == defer
    a.close(); b.close()


# ---- 5. place equals the two hops -------------------------------------------------------------------------------------------------------------------------
TARGETS = [(8, 0, 0), (24, -24, 16), (64, 0, 0), (-72, 8, 0), (0, 0, 0)]
PLACE_CASES = [(64, False, o) for o in TARGETS] + [(72, False, (24, -24, 16)), (72, False, (-72, 8, 0)), (64, True, (24, -24, 16)), (64, True, (0, 0, 0))]


@pytest.mark.parametrize("res,color,target", PLACE_CASES)
def test_place_equals_the_two_hops(res, color, target):
    a, b = G.make_ctx(res, color, 300000), G.make_ctx(res, color, 300000)
    for ctx in (a, b):
        ctx.set_defer(1)
        ctx.brick_store_reserve(CAP)
        G.fuse(ctx, range(6), color)
    before = planes_bits(a, color)
    pose = G.pose_of(a)
    a.place_window(*target)
    b.brick_store_capture()
    b.shift_volume(target[0] + 4 * res, target[1], target[2])     # a frame that overlaps neither window
    b.shift_volume(-4 * res, 0, 0)
    assert np.array_equal(u32(G.pose_of(a)), u32(G.moved_pose(pose, target, a.size / res)))
    assert same_planes(a, b, color)
    assert a.stats()["weight_gt0"] == b.stats()["weight_gt0"] and a.volume_origin() == b.volume_origin() == tuple(target)
    assert same_store(B.store_sorted(a), B.store_sorted(b)) and a.brick_store_count() == b.brick_store_count()
    assert a.brick_store_count()[0] >= 100
    if target == (0, 0, 0):
        assert equal_bits(planes_bits(a, color), before)           # everything came back, the deferred-weight words with it
    # derived state: B's two translations round twice, so both get A's pose, then the same raycast, extraction and frames
    pa = G.pose_of(a)
    for ctx in (a, b):
        ctx.set_pose(pa)
        G.raycast(ctx, color)
    G.assert_same_model(a, b, color)
    thr = 300 * a.size / res
    a.marching_cubes(thr, has_color=color)
    b.marching_cubes(thr, has_color=color)
    ta, tb = a.triangles(), b.triangles()
    assert G.same_bits(ta, tb) and (len(ta) > 1000 or target[0] >= 64 or target[0] <= -64)
    for k in range(6, 10):
        oka, qa = G.run_frame(a, k, color)
        okb, qb = G.run_frame(b, k, color)
        assert oka == okb and np.array_equal(u32(qa), u32(qb)), (k, qa, qb)
        assert same_planes(a, b, color), k
        assert color or a.fusion_form()["defer"] == 1             # (the colour fusion pass has no deferred form)
    a.close(); b.close()


def test_placing_at_the_current_origin_changes_no_later_frame():
    a, b = G.make_ctx(64), G.make_ctx(64)
    for ctx in (a, b):
        ctx.set_defer(1)
        ctx.brick_store_reserve(CAP)
        G.fuse(ctx, range(6))
    a.place_window(0, 0, 0)
    G.raycast(a); G.raycast(b)
    assert same_planes(a, b) and np.array_equal(u32(G.pose_of(a)), u32(G.pose_of(b)))
    for k in range(6, 10):
        oka, pa = G.run_frame(a, k)
        okb, pb = G.run_frame(b, k)
        assert oka and okb and np.array_equal(u32(pa), u32(pb)), (k, pa, pb)
        assert same_planes(a, b), k
        assert a.fusion_form()["defer"] == 1
    a.close(); b.close()


# ---- 6. place with a store too small ----------------------------------------------------------------------------------------------------------------------
def test_place_with_a_store_too_small():
    ctx = B.fused_ctx(64, cap=8)
    planes, pose = planes_bits(ctx), G.pose_of(ctx)
    assert ctx.lib.kf_place_window(ctx.h, 24, -24, 16) == ALLOC
    assert equal_bits(planes_bits(ctx), planes) and ctx.volume_origin() == (0, 0, 0) and np.array_equal(u32(G.pose_of(ctx)), u32(pose))
    held, dropped, restored = ctx.brick_store_count()
    assert held == 8 and dropped >= 92 and restored == 0
    ok, _ = G.run_frame(ctx, 6)                                    # ... and the session goes on
    assert ok
    ctx.close()


# ---- 7. save, load, go on -----------------------------------------------------------------------------------------------------------------------------------
_VGA = {}


def app_frame(app, k, size, cam, color):
    if color and (k, size) not in _VGA:
        _VGA[(k, size)] = np.ascontiguousarray(S.render_depth_mm(S.trajectory_pose(k, size), cam, size), np.uint16)
    mm = _VGA[(k, size)] if color else G.frame(k, size)
    if color:
        y, x = np.mgrid[0:cam[1], 0:cam[0]]
        rgb = np.ascontiguousarray(np.stack([(x * 3 + k * 7) % 256, (y * 5 + x) % 256, (x + 2 * y + 31 * k) % 256], axis=-1).astype(np.uint8))
        return app.h.hkf_app_process_frame_color(mm.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), k, C.c_double(0.0)) == 1
    return app.process_frame(mm, k)


def make_app(res, size, cam, color):
    return H.App(res, size, cam, max_triangles=300000, sdf_trunc=5 * size / res, integrate_dist=G.GATE, use_rgb=color)


def app_state(app, ctx, color):
    ok, pose = app.pose()
    return ok, u32(pose).copy(), planes_bits(ctx, color)


def map_pictures(app, ctx, res, size, cam, color, world_pose):
    ctx.clear_triangles()
    ctx.marching_cubes_map(300 * size / res, has_color=color)
    tris = ctx.triangles().tobytes()
    return tris, app.render_map_view(K.VIEW_COLOR if color else K.VIEW_SHADED, world_pose, cam).tobytes()


@pytest.mark.parametrize("res,color", CASES)
def test_save_load_go_on(tmp_path, res, color):
    """the colour application fuses with the VGA camera for depth and colour alike (the host class gives both cameras the same intrinsics, and the fusion pass
    projects colour with the VGA ones)"""
    size = G.SIZES[res]
    cam = G.RGB_CAM if color else G.CAM
    path = str(tmp_path / "session.hkfmap")
    a = make_app(res, size, cam, color)
    try:
        a.set_brick_store(CAP)
        ca = K.Context.borrow(a.ctx_handle(), K.camera(*cam), res, size)
        for k in range(6):
            assert app_frame(a, k, size, cam, color), k
            if k == 2:
                assert a.shift_volume(32, 0, 0)
        in_store = a.brick_store_count()[0]
        in_window = np.count_nonzero(G.planes(ca, color)[1] > 0)
        assert in_store > 0 and in_window > 0
        assert a.save_map(path)
        saved = dict(origin=a.volume_origin(), frame_id=a.frame_id(), held=a.brick_store_count()[0])
        assert saved["origin"] == (32, 0, 0) and saved["frame_id"] == 5 and saved["held"] > in_store and a.brick_store_count()[1] == 0
        info = H.map_file_info(path)
        assert (info["resolution"], info["has_color"], info["origin_vox"], info["frame_id"], info["n_bricks"], info["dropped"]) == \
            (res, color, (32, 0, 0), 5, saved["held"], 0)
        world_pose = a.pose()[1].copy()
        world_pose[:3, 3] += np.float32(32 * size / res) * np.array([1, 0, 0], np.float32)
        pictures = map_pictures(a, ca, res, size, cam, color, world_pose)
        assert len(pictures[0]) > 1000 * 72
        trace = []
        for k in range(6, 10):
            assert app_frame(a, k, size, cam, color), k
            trace.append(app_state(a, ca, color))
    finally:
        a.close()
    b = make_app(res, size, cam, color)
    try:
        assert b.load_map(path)
        cb = K.Context.borrow(b.ctx_handle(), K.camera(*cam), res, size)
        assert b.volume_origin() == saved["origin"] and b.frame_id() == saved["frame_id"] and b.brick_store_count()[0] == saved["held"]
        got = map_pictures(b, cb, res, size, cam, color, world_pose)
        assert got[0] == pictures[0] and got[1] == pictures[1]
        for k in range(6, 10):
            assert app_frame(b, k, size, cam, color), k           # tracked against the loaded model, not treated as a first frame
            ok, pose, planes = app_state(b, cb, color)
            assert ok == trace[k - 6][0] and np.array_equal(pose, trace[k - 6][1]), k
            assert equal_bits(planes, trace[k - 6][2]), k
    finally:
        b.close()


# ---- 8. the file depends on the map alone -----------------------------------------------------------------------------------------------------------------------
def test_the_file_depends_on_the_map_alone(tmp_path):
    res, size = 64, 2.0
    p1, p2 = str(tmp_path / "here.hkfmap"), str(tmp_path / "there.hkfmap")
    a = make_app(res, size, G.CAM, False)
    try:
        a.set_brick_store(CAP)
        for k in range(6):
            assert app_frame(a, k, size, G.CAM, False), k
            if k == 2:
                assert a.shift_volume(32, 0, 0)
        assert a.save_map(p1)
        ctx = K.Context.borrow(a.ctx_handle(), K.camera(*G.CAM), res, size)
        ctx.place_window(0, 32, 0)                                # half a window away, in both axes
        assert a.save_map(p2)
    finally:
        a.close()
    d1, d2 = open(p1, "rb").read(), open(p2, "rb").read()
    assert len(d1) == len(d2) and len(d1) > 128 + 100 * 4108 and d1[128:] == d2[128:]
    i1, i2 = H.map_file_info(p1), H.map_file_info(p2)
    assert i1["origin_vox"] == (32, 0, 0) and i2["origin_vox"] == (0, 32, 0)
    assert np.array_equal(u32(i2["pose"]), u32(G.moved_pose(i1["pose"], (-32, 32, 0), size / res)))
    differing = {i for i in range(128) if d1[i] != d2[i]}
    assert differing and differing <= set(range(32, 44)) | set(range(48 + 12, 48 + 16)) | set(range(48 + 28, 48 + 32)) | set(range(48 + 44, 48 + 48))


# ---- 9. load refuses a foreign map ------------------------------------------------------------------------------------------------------------------------------------
def test_load_refuses_a_foreign_map(tmp_path):
    size = 2.0
    paths = {}
    for name, res, color in (("own", 64, False), ("res72", 72, False), ("colour", 64, True)):
        cam = G.RGB_CAM if color else G.CAM
        app = make_app(res, G.SIZES[res], cam, color)
        try:
            app.set_brick_store(CAP)
            for k in range(2):
                assert app_frame(app, k, G.SIZES[res], cam, color), k
            paths[name] = str(tmp_path / (name + ".hkfmap"))
            assert app.save_map(paths[name])
        finally:
            app.close()
    own = open(paths["own"], "rb").read()
    for name, data in (("cut", own[:-1]), ("magic", b"X" + own[1:]), ("flag", own[:20] + b"\x01" + own[21:])):
        paths[name] = str(tmp_path / (name + ".hkfmap"))
        with open(paths[name], "wb") as f:
            f.write(data)
    b = make_app(64, size, G.CAM, False)
    try:
        b.set_brick_store(CAP)
        for k in range(3):
            assert app_frame(b, k, size, G.CAM, False), k
        assert b.shift_volume(32, 0, 0)
        cb = K.Context.borrow(b.ctx_handle(), K.camera(*G.CAM), 64, size)
        planes, store, counts = planes_bits(cb), B.store_sorted(cb), b.brick_store_count()
        assert counts[0] > 0
        for name in ("res72", "colour", "cut", "magic", "flag", "missing"):
            assert not b.load_map(paths.get(name, str(tmp_path / "missing.hkfmap"))), name
            assert equal_bits(planes_bits(cb), planes) and same_store(B.store_sorted(cb), store) and b.brick_store_count() == counts, name
            assert b.volume_origin() == (32, 0, 0) and b.frame_id() == 2
        assert b.load_map(paths["own"]) and b.volume_origin() == (0, 0, 0) and b.frame_id() == 1      # ... and takes its own
    finally:
        b.close()
