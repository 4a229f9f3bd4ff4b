"""GPU: the brick store.  With a store reserved, kf_shift_volume keeps every observed brick that leaves the window and restores every brick that
enters and is found, so a shift away and back is lossless.  The expectation is a numpy model: a dict from world brick coordinate to brick contents,
filled from the planes downloaded before each shift and applied to the numpy slice-and-zero of those planes.  Everything is compared as integers,
bit for bit.  Shapes, stream and helpers are those of test_gpu_shift.py: 64 voxels at 2.0 m and 72 at 2.25 m (cell 1 / 32; 72 gives ragged tables),
a 160 x 120 camera, 6 fused frames of Scene S, colour with the VGA colour camera.

A shift of 8 along x evicts no observed brick of Scene S at these sizes (the observed bricks span brick indices 1-6 in x and y), so the shifts are
larger: each test counts, from the downloaded planes, the observed bricks that leave and how many of them hold a negative tsdf."""
import numpy as np
import pytest

import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32 = np.float32
SHIFTS = [(24, -24, 16), (32, 0, 0), (0, 0, -16), (0, 0, 16)]     # the last two: the back wall leaves / free space in front of the camera leaves
CASES = [(64, False), (72, False), (64, True)]
CAP = 1024


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bricks(a):
    """planes (R, R, R[, 3]) in (z, y, x) order -> a view [bz, by, bx] of (8, 8, 8[, 3]) bricks in (z, y, x) order"""
    nb = a.shape[0] // 8
    if a.ndim == 4:
        return a.reshape(nb, 8, nb, 8, nb, 8, 3).transpose(0, 2, 4, 1, 3, 5, 6)
    return a.reshape(nb, 8, nb, 8, nb, 8).transpose(0, 2, 4, 1, 3, 5)


class Model:
    """what the store must hold and what a shift must produce"""

    def __init__(self):
        self.store = {}                                           # (x, y, z) world brick coordinate -> (tsdf, weight, colour or None)
        self.origin = np.zeros(3, np.int64)                       # voxels
        self.restored = 0

    def shift(self, t, w, c, d):
        """the planes after a shift by d of a window holding (t, w, c); returns (t, w, c, observed bricks that left, of them with a negative tsdf)"""
        nb = t.shape[0] // 8
        s = [x // 8 if x >= 0 else -((-x) // 8) for x in d]
        tb, wb, cb = bricks(t), bricks(w), bricks(c) if c is not None else None
        ob = self.origin // 8
        n_obs = n_neg = 0
        for bz in range(nb):
            for by in range(nb):
                for bx in range(nb):
                    b = (bx, by, bz)
                    if all(0 <= b[k] - s[k] < nb for k in range(3)) or not np.any(wb[bz, by, bx] > 0):
                        continue
                    n_obs += 1
                    n_neg += bool(np.any(tb[bz, by, bx] < 0))
                    self.store[tuple(int(ob[k] + b[k]) for k in range(3))] = (tb[bz, by, bx].copy(), wb[bz, by, bx].copy(),
                                                                               cb[bz, by, bx].copy() if cb is not None else None)
        t, w = G.np_shift(t, d), G.np_shift(w, d)
        c = G.np_shift(c, d) if c is not None else None
        self.origin = self.origin + np.array(d, np.int64)
        ob = self.origin // 8
        tb, wb, cb = bricks(t), bricks(w), bricks(c) if c is not None else None
        for bz in range(nb):
            for by in range(nb):
                for bx in range(nb):
                    b = (bx, by, bz)
                    if all(0 <= b[k] + s[k] < nb for k in range(3)):
                        continue
                    hit = self.store.get(tuple(int(ob[k] + b[k]) for k in range(3)))
                    if hit is None:
                        continue
                    self.restored += 1
                    tb[bz, by, bx], wb[bz, by, bx] = hit[0], hit[1]
                    if cb is not None:
                        cb[bz, by, bx] = hit[2]
        return t, w, c, n_obs, n_neg

    def sorted(self):
        keys = sorted(self.store, key=lambda k: (k[2], k[1], k[0]))
        return (np.array(keys, np.int32).reshape(-1, 3), np.stack([self.store[k][0] for k in keys]), np.stack([self.store[k][1] for k in keys]),
                np.stack([self.store[k][2] for k in keys]) if keys and self.store[keys[0]][2] is not None else None)


def store_sorted(ctx):
    keys, t, w, c = ctx.brick_store()
    o = np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))
    return keys[o], t[o], w[o], c[o] if c is not None else None


def assert_planes(ctx, color, t, w, c, what):
    gt, gw, gc = G.planes(ctx, color)
    assert np.array_equal(u32(gt), u32(t)), what                  # as integers: -0.0 cannot hide
    assert np.array_equal(u32(gw), u32(w)), what
    if color:
        assert np.array_equal(gc, c), what
    assert ctx.stats()["weight_gt0"] == np.count_nonzero(w > 0), what


def assert_store(ctx, model, what):
    held, dropped, restored = ctx.brick_store_count()
    assert (held, dropped, restored) == (len(model.store), 0, model.restored), what
    gk, gt, gw, gc = store_sorted(ctx)
    mk, mt, mw, mc = model.sorted()
    assert np.array_equal(gk, mk), what
    assert np.array_equal(u32(gt), u32(mt)) and np.array_equal(u32(gw), u32(mw)), what
    if mc is not None:
        assert np.array_equal(gc, mc), what


def fused_ctx(res, color=False, cap=CAP, **kw):
    ctx = G.make_ctx(res, color, **kw)
    if cap:
        ctx.brick_store_reserve(cap)
    G.fuse(ctx, range(6), color)
    return ctx


# ---- 1. there and back ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_there_and_back(res, color):
    ctx = fused_ctx(res, color)
    model = Model()
    assert ctx.brick_store_count() == (0, 0, 0)
    for d in SHIFTS:
        t0, w0, c0 = G.planes(ctx, color)
        t1, w1, c1, n_obs, n_neg = model.shift(t0, w0, c0, d)
        print(res, color, d, "observed bricks leaving", n_obs, "with a negative tsdf", n_neg, "bricks held", len(model.store))
        assert n_obs >= 20 and (n_neg >= 10 or d == (0, 0, 16)), (d, n_obs, n_neg)      # (free space in front of the camera holds little surface)
        ctx.shift_volume(*d)
        assert_planes(ctx, color, t1, w1, c1, d)
        assert_store(ctx, model, d)
        assert ctx.volume_origin() == tuple(d)
        back = tuple(-x for x in d)
        t2, w2, c2, _, _ = model.shift(t1, w1, c1, back)
        assert np.array_equal(u32(t2), u32(t0)) and np.array_equal(u32(w2), u32(w0))    # the model itself is lossless
        ctx.shift_volume(*back)
        assert_planes(ctx, color, t0, w0, c0, back)
        assert_store(ctx, model, back)
        assert ctx.volume_origin() == (0, 0, 0)
    assert model.restored >= 80
    ctx.close()


# ---- 2. everything leaves and returns -------------------------------------------------------------------------------------------------------
def test_everything_leaves_and_returns():
    ctx = fused_ctx(64)
    t0, w0, _ = G.planes(ctx)
    n_obs = int(np.count_nonzero(np.any(bricks(w0).reshape(8, 8, 8, 512) > 0, axis=-1)))
    print("observed bricks", n_obs)
    assert n_obs >= 100
    ctx.shift_volume(64, 0, 0)
    t1, w1, _ = G.planes(ctx)
    assert not np.any(t1) and not np.any(w1)
    assert ctx.brick_store_count() == (n_obs, 0, 0)
    ctx.shift_volume(-64, 0, 0)
    assert_planes(ctx, False, t0, w0, None, "back")
    assert ctx.brick_store_count() == (n_obs, 0, n_obs)
    ctx.close()


# ---- 3. derived state after a partial return -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_derived_state_after_a_partial_return(res, color):
    """A shifts away and half-way back: some bricks move, some are restored.  B, fresh, gets the model's planes uploaded and A's pose.  A restored
    brick whose has-negative bit or macro mark was missed shows in the raycast or in the extraction."""
    a = G.make_ctx(res, color, 300000)
    b = G.make_ctx(res, color, 300000)
    a.brick_store_reserve(CAP)
    G.fuse(a, range(6), color)
    model = Model()
    t, w, c = G.planes(a, color)
    t, w, c, n_obs, n_neg = model.shift(t, w, c, (32, 0, 0))
    assert n_obs >= 20 and n_neg >= 10
    t, w, c, _, _ = model.shift(t, w, c, (-16, 0, 0))
    assert model.restored >= 10
    a.shift_volume(32, 0, 0)
    a.shift_volume(-16, 0, 0)
    assert a.brick_store_count()[2] == model.restored
    b.upload_volume(t, w, c)
    b.set_pose(G.pose_of(a))
    G.raycast(a, color)
    G.raycast(b, color)
    G.assert_same_model(a, b, color)
    thr = 300 * a.size / res
    a.marching_cubes(thr, has_color=color)
    b.marching_cubes(thr, has_color=color)
    ta, tb = a.triangles(), b.triangles()
    assert len(ta) > 1000 and G.same_bits(ta, tb)
    assert_planes(a, color, t, w, c, "partial return")
    a.close(); b.close()


# ---- 4. going on, with deferral ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 72])
def test_going_on_with_deferral(res):
    """A defers whole-quarter free-space weights and takes the round trip through the store; B never defers and gets A's planes and pose afterwards.
    The deferred-weight words must come back with their bricks: frames 6-9 give the same pose bits and the same planes."""
    a, b = G.make_ctx(res), G.make_ctx(res)
    a.set_defer(1); b.set_defer(0)
    a.brick_store_reserve(CAP)
    G.fuse(a, range(6))
    assert a.fusion_form()["defer"] == 1
    t0, w0, _ = G.planes(a)
    a.shift_volume(0, -24, 16)
    a.shift_volume(0, 24, -16)
    held, dropped, restored = a.brick_store_count()
    assert held >= 20 and dropped == 0 and restored == held
    t, w, _ = G.planes(a)
    assert np.array_equal(u32(t), u32(t0)) and np.array_equal(u32(w), u32(w0))
    b.upload_volume(t, w)
    b.set_pose(G.pose_of(a))
    G.raycast(a); G.raycast(b)
    for k in range(6, 10):
        oka, pa = G.run_frame(a, k)
        okb, pb = G.run_frame(b, k)
        assert oka and okb, k
        assert np.array_equal(u32(pa), u32(pb)), (k, pa, pb)
        assert a.fusion_form()["defer"] == 1 and b.fusion_form()["defer"] == 0
    ta, wa, _ = G.planes(a)
    tb, wb, _ = G.planes(b)
    assert np.array_equal(u32(ta), u32(tb)) and np.array_equal(u32(wa), u32(wb))
    a.close(); b.close()


# ---- 5. re-departure overwrites ----------------------------------------------------------------------------------------------------------------
def test_re_departure_overwrites():
    ctx = fused_ctx(64)
    model = Model()
    d, back = (0, 0, -16), (0, 0, 16)
    t, w, _ = G.planes(ctx)
    for s in (d, back):
        t, w, _, _, _ = model.shift(t, w, None, s)
        ctx.shift_volume(*s)
    G.raycast(ctx)
    first = {k: v[1].copy() for k, v in model.store.items()}
    for k in range(6, 10):
        ok, _ = G.run_frame(ctx, k)
        assert ok, k
    t0, w0, _ = G.planes(ctx)
    t, w = t0, w0
    for s in (d, back):
        t, w, _, n_obs, _ = model.shift(t, w, None, s)
        ctx.shift_volume(*s)
        if s == d:
            assert n_obs >= 20
    assert set(first) <= set(model.store)                         # the same keys leave again ...
    assert sum(not np.array_equal(first[k], model.store[k][1]) for k in first) >= 10    # ... with what frames 6-9 added: the entries must be overwritten
    assert_planes(ctx, False, t0, w0, None, "second round trip")
    assert_store(ctx, model, "second round trip")                 # held == the model's size: no key took a second slot
    ctx.close()


# ---- 6. a full store -----------------------------------------------------------------------------------------------------------------------------
def test_a_full_store_drops_and_misses():
    ctx = fused_ctx(64, cap=32)
    d = (24, -24, 16)
    t0, w0, _ = G.planes(ctx)
    model = Model()
    _, _, _, n_obs, _ = model.shift(t0, w0, None, d)
    assert n_obs >= 64
    ctx.shift_volume(*d)
    assert ctx.brick_store_count() == (32, n_obs - 32, 0)
    keys = ctx.brick_store()[0]
    assert len({tuple(k) for k in keys.tolist()}) == 32 and all(tuple(k) in model.store for k in keys.tolist())
    ctx.shift_volume(*[-x for x in d])
    t1, w1, _ = G.planes(ctx)
    same = np.all(u32(bricks(t1)).reshape(8, 8, 8, 512) == u32(bricks(t0)).reshape(8, 8, 8, 512), axis=-1) & \
        np.all(u32(bricks(w1)).reshape(8, 8, 8, 512) == u32(bricks(w0)).reshape(8, 8, 8, 512), axis=-1)
    zero = ~np.any(u32(bricks(t1)).reshape(8, 8, 8, 512), axis=-1) & ~np.any(u32(bricks(w1)).reshape(8, 8, 8, 512), axis=-1)
    assert np.all(same | zero)
    departed = np.zeros((8, 8, 8), bool)                          # [bz, by, bx]: the observed bricks that left
    for (x, y, z) in model.store:
        departed[z, y, x] = True
    assert np.count_nonzero(departed) == n_obs and np.count_nonzero(departed & same) == 32 and np.count_nonzero(departed & zero) == n_obs - 32
    assert ctx.brick_store_count() == (32, n_obs - 32, 32)
    ctx.brick_store_reserve(CAP)                                  # a second reserve empties the store
    assert ctx.brick_store_count() == (0, 0, 0) and len(ctx.brick_store()[0]) == 0
    ctx.close()


# ---- 7. stream-out is untouched -------------------------------------------------------------------------------------------------------------------
def test_stream_out_is_untouched():
    res = 64
    thr = 300 * G.SIZES[res] / res
    a, b = G.make_ctx(res, False, 300000), G.make_ctx(res, False, 300000)
    a.brick_store_reserve(CAP)
    for ctx in (a, b):
        ctx.world_soup_reserve(200000)
        ctx.set_stream_out(True, thr)
        G.fuse(ctx, range(6))
        ctx.shift_volume(32, 0, 0)
    sa, sb = a.world_soup(), b.world_soup()
    assert len(sa) > 1000 and a.world_soup_count() == b.world_soup_count() and G.same_bits(sa, sb)
    ta, wa, _ = G.planes(a)
    tb, wb, _ = G.planes(b)
    assert np.array_equal(u32(ta), u32(tb)) and np.array_equal(u32(wa), u32(wb))
    assert a.brick_store_count()[0] >= 20 and b.brick_store_count() == (0, 0, 0)
    a.close(); b.close()


# ---- 8. refusals and the off path --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_off_path():
    res = 64
    slab = G.make_ctx(res, slab=(0, 32), halo=8)
    assert slab.lib.kf_brick_store_reserve(slab.h, 64) == 1001    # KF_ERR_ARG: a z-slab context cannot shift
    slab.close()
    ctx = G.make_ctx(res)
    assert ctx.lib.kf_brick_store_clear(ctx.h) == 1002            # KF_ERR_STATE: no store
    assert ctx.brick_store_count() == (0, 0, 0)
    ctx.brick_store_reserve(CAP)
    G.fuse(ctx, range(6))
    assert ctx.lib.kf_read_brick_store(ctx.h, 0, 1, None, None, None, None) == 1001       # nothing held yet
    ctx.shift_volume(0, 0, -16)
    held = ctx.brick_store_count()[0]
    assert held >= 20
    assert ctx.lib.kf_read_brick_store(ctx.h, 0, held, None, None, None, None) == 0
    assert ctx.lib.kf_read_brick_store(ctx.h, 1, held, None, None, None, None) == 1001    # past `held`
    assert ctx.lib.kf_read_brick_store(ctx.h, held, 0, None, None, None, None) == 0
    ctx.shift_volume(0, 0, 16)
    # one large legal shift (it empties the window): the window's last brick then has world coordinate 2^20 - 1 along x
    far = 8 * ((1 << 20) - res // 8)
    ctx.shift_volume(far, 0, 0)
    assert ctx.volume_origin() == (far, 0, 0)
    t, w = ctx.download_volume()
    assert not np.any(t) and not np.any(w)
    pose, counts = G.pose_of(ctx), ctx.brick_store_count()
    assert ctx.lib.kf_shift_volume(ctx.h, 8, 0, 0) == 1001        # the new window would cross 2^20
    assert ctx.lib.kf_shift_volume(ctx.h, 8, -8, 16) == 1001
    t2, w2 = ctx.download_volume()
    assert np.array_equal(u32(t2), u32(t)) and np.array_equal(u32(w2), u32(w))
    assert np.array_equal(u32(G.pose_of(ctx)), u32(pose)) and ctx.volume_origin() == (far, 0, 0) and ctx.brick_store_count() == counts
    assert ctx.lib.kf_shift_volume(ctx.h, 0, 8, 8) == 0           # (the other axes are free)
    assert ctx.volume_origin() == (far, 8, 8)
    ctx.brick_store_reserve(0)                                    # without a store the same shift is legal again
    assert ctx.lib.kf_shift_volume(ctx.h, 8, 0, 0) == 0 and ctx.volume_origin() == (far + 8, 8, 8)
    ctx.close()
    # the off path: after brick_store_reserve(0) a shift away and back leaves zeros where the bricks left, as it always did
    ctx = fused_ctx(res)
    ctx.brick_store_reserve(0)
    t0, w0, _ = G.planes(ctx)
    d = (0, 0, -16)
    ctx.shift_volume(*d)
    ctx.shift_volume(0, 0, 16)
    assert_planes(ctx, False, G.np_shift(G.np_shift(t0, d), (0, 0, 16)), G.np_shift(G.np_shift(w0, d), (0, 0, 16)), None, "off")
    assert np.count_nonzero(w0 > 0) - ctx.stats()["weight_gt0"] > 1000 and ctx.brick_store_count() == (0, 0, 0)
    ctx.close()


# ---- 9. the host class ------------------------------------------------------------------------------------------------------------------------------
def host_round_trip(store):
    size, res = 2.0, 64
    app = H.App(res, size, G.CAM, sdf_trunc=5 * size / res, integrate_dist=G.GATE)
    if store:
        app.set_brick_store(CAP)
    for k in range(4):
        assert app.process_frame(G.frame(k, size), k)
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*G.CAM), res, size)
    before = ctx.download_volume()
    assert app.shift_volume(0, 0, -16) and app.shift_volume(0, 0, 16)
    after = ctx.download_volume()
    counts = app.brick_store_count()
    tracked = [app.process_frame(G.frame(k, size), k) for k in range(4, 7)]
    app.close()
    return before, after, counts, tracked


def test_host_class_round_trip():
    before, after, counts, tracked = host_round_trip(True)
    assert np.array_equal(u32(after[0]), u32(before[0])) and np.array_equal(u32(after[1]), u32(before[1]))
    assert counts[0] >= 20 and counts[1] == 0 and counts[2] == counts[0]
    assert all(tracked)
    _, twin_after, twin_counts, _ = host_round_trip(False)
    assert twin_counts == (0, 0, 0)
    assert np.count_nonzero(twin_after[1] > 0) < np.count_nonzero(after[1] > 0)
