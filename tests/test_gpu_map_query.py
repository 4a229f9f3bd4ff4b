"""GPU: querying the map.  kf_map_sample reads tsdf, gradient, weight and colour at points, kf_map_cast_rays marches rays to their first surface crossing --
both through the window and, outside it, the brick store, where they lie.  The yardstick is tests/map_query_expect.py (np_sample, np_cast: the definition
in include/hybkf.h restated in numpy), held against closed forms by tests/test_map_query_cpu.py, which also shows that the point and ray sets used here hold
enough of every kind.  Shapes, stream and helpers are those of test_gpu_brickstore.py and test_gpu_shift.py: 64 voxels at 2.0 m and 72 at 2.25 m, colour at
64, the 160 x 120 camera, 6 fused frames of Scene S, a store of 1024 bricks.  Everything is compared as integers, bit for bit."""
import functools

import numpy as np
import pytest

import map_query_expect as E
import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
f32 = np.float32
CAP = B.CAP
CASES = B.CASES
ARG, STATE = 1001, 1002
SAMPLE_KEYS = ("tsdf", "weight", "grad", "color")
CAST_KEYS = ("status", "t", "normal", "color", "weight")
SHIFT = (-24, 16, 8)                                              # the mixed cases: the surface partly in the window, partly in the store


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (what, k, int(np.count_nonzero(bits(got[k]) != bits(want[k]))))


def strip_color(bricks, color):
    return bricks if color else {k: (t, w, None) for k, (t, w, c) in bricks.items()}


def write_map(ctx, bricks, color):
    keys = sorted(bricks)
    assert len(keys) <= CAP
    ctx.write_brick_store(np.array(keys, np.int32), np.stack([bricks[k][0] for k in keys]), np.stack([bricks[k][1] for k in keys]),
                          np.stack([bricks[k][2] for k in keys]) if color else None)
    assert ctx.brick_store_count()[:2] == (len(keys), 0)


def store_only_ctx(res, color, bricks):
    """an otherwise empty context whose store holds the map and whose window stands far away from it"""
    ctx = G.make_ctx(res, color)
    ctx.brick_store_reserve(CAP)
    ctx.shift_volume(0, 0, -4096)
    write_map(ctx, bricks, color)
    return ctx


def map_dict(ctx, color, store=True):
    """the dictionary of a context, window first: the sorted store read-out, then EVERY brick of the window laid over it -- observed or not, the window's
    copy is the map there.  Returns (dictionary, the window's keys)"""
    d = {}
    if store:
        keys, t, w, c = B.store_sorted(ctx)
        for i, k in enumerate(keys):
            d[tuple(int(v) for v in k)] = (t[i], w[i], c[i] if c is not None else None)
    o = ctx.volume_origin()
    assert all(v % 8 == 0 for v in o)
    t, w, c = G.planes(ctx, color)
    tb, wb, cb = B.bricks(t), B.bricks(w), B.bricks(c) if c is not None else None
    nb = ctx.res // 8
    window = set()
    for bz in range(nb):
        for by in range(nb):
            for bx in range(nb):
                k = (o[0] // 8 + bx, o[1] // 8 + by, o[2] // 8 + bz)
                d[k] = (tb[bz, by, bx], wb[bz, by, bx], cb[bz, by, bx] if cb is not None else None)
                window.add(k)
    return d, window


@functools.lru_cache(maxsize=None)
def sphere_expected(color):
    m = E.MapIndex(strip_color(E.sphere_map(), color))
    return E.np_sample(m, E.sphere_points()), E.np_cast(m, *E.sphere_rays(), E.STEP)


@functools.lru_cache(maxsize=None)
def plane_expected(color):
    m = E.MapIndex(strip_color(E.plane_map(), color))
    return E.np_cast(m, *E.plane_rays(), E.STEP)


# ---- 1. analytic maps, at the origin and at far keys ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("res,color", CASES)
def test_analytic_maps(res, color, far):
    db = E.FAR if far else (0, 0, 0)
    want_s, want_r = sphere_expected(color)
    pts, (o, d, t0, t1) = E.sphere_points(), E.sphere_rays()
    ctx = store_only_ctx(res, color, E.shifted(E.sphere_map(), db))
    body = slice(0, len(pts) - E.N_ODD)
    q = pts.copy()
    q[body] = E.moved(pts[body], db)
    got = ctx.map_sample(q)
    if far:                                                       # the odd points stay where they are: they have their own expectation
        want_s = dict(want_s)
        odd = E.np_sample(strip_color(E.shifted(E.sphere_map(), db), color), q[len(pts) - E.N_ODD:])
        for k in SAMPLE_KEYS:
            want_s[k] = np.concatenate([want_s[k][body], odd[k]])
    assert_same(got, want_s, SAMPLE_KEYS, ("sphere points", far))
    assert np.count_nonzero(got["weight"]) >= 1024 and (not color or np.count_nonzero(got["color"]) > 1000)
    got = ctx.map_cast_rays(E.moved(o, db), d, t0, t1, E.STEP)
    assert_same(got, want_r, CAST_KEYS, ("sphere rays", far))
    assert np.count_nonzero(got["status"] == K.RAY_HIT) >= 1024 and np.count_nonzero(got["status"] == K.RAY_BROKEN) >= 32
    if not far:                                                   # the same map seen through the window: placed over it, the window answers
        ctx.place_window(0, 0, 0)
        assert ctx.volume_origin() == (0, 0, 0)
        assert_same(ctx.map_sample(pts), want_s, SAMPLE_KEYS, "sphere points, window")
        assert_same(ctx.map_cast_rays(o, d, t0, t1, E.STEP), want_r, CAST_KEYS, "sphere rays, window")
    ctx.close()
    ctx = store_only_ctx(res, color, E.shifted(E.plane_map(), db))
    o, d, t0, t1 = E.plane_rays()
    got = ctx.map_cast_rays(E.moved(o, db), d, t0, t1, E.STEP)
    assert_same(got, plane_expected(color), CAST_KEYS, ("plane rays", far))
    assert (got["status"] == K.RAY_HIT).all()
    ctx.close()


# ---- 2. mixed sources, deferred weights, no store --------------------------------------------------------------------------------------------------------
def camera_rays(pose, cam, cell, origin, every=4):
    """the pose's camera rays in world voxels: the camera at pose_t / cell + origin, directions R ((u - cx) / fx, (v - cy) / fy, 1) normalised in fp32"""
    cols, rows, cx, cy, fx, fy = cam
    v, u = np.mgrid[0:rows, 0:cols]
    u, v = u.reshape(-1)[::every], v.reshape(-1)[::every]
    local = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones(len(u))], axis=1)
    local /= np.linalg.norm(local, axis=1, keepdims=True)
    d = (local @ np.asarray(pose, np.float64)[:3, :3].T).astype(f32)
    o = np.asarray(pose, np.float64)[:3, 3] / float(cell) + np.asarray(origin, np.float64)
    return np.broadcast_to(o, (len(d), 3)).copy(), d


def mixed_ctx(res, color, defer=None, max_weight=None, store=True):
    """6 fused frames, captured, the window shifted: what left is in the store, what stayed or came back is the window's"""
    if max_weight is None:
        ctx = G.make_ctx(res, color)
    else:
        ctx = K.Context(K.camera(*G.CAM), res, G.SIZES[res], max_weight, levels=3)
    if defer is not None:
        ctx.set_defer(defer)
    if store:
        ctx.brick_store_reserve(CAP)
    G.fuse(ctx, range(6), color)
    if store:
        ctx.brick_store_capture()
    ctx.shift_volume(*SHIFT)
    G.raycast(ctx, color)
    return ctx


def mixed_queries(ctx, window, idx):
    """points: every voxel centre of four window bricks that touch the window's +x face and have a store brick beyond it, points exactly on that face, 4 096
    random points; rays: the pose's camera rays (every 4th) and 512 rays from over the store into the window"""
    rng = np.random.default_rng(41)
    res, o = ctx.res, np.array(ctx.volume_origin())
    cell = f32(ctx.size) / f32(res)
    held = set(map(tuple, idx.keys.tolist()))
    face_b = (o[0] + res) // 8                                    # the first brick layer beyond the face
    cut = [k for k in sorted(window) if k[0] == face_b - 1 and (face_b, k[1], k[2]) in held and (face_b, k[1], k[2]) not in window
           and np.any(idx.w[np.flatnonzero(np.all(idx.keys == k, axis=1))[0]] > 0)]
    assert len(cut) >= 4, len(cut)
    cut = cut[:: max(1, len(cut) // 4)][:4]
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    centres = np.concatenate([np.stack([8 * k[0] + x, 8 * k[1] + y, 8 * k[2] + z], axis=-1).reshape(-1, 3) + 0.5 for k in cut])
    on_face = np.concatenate([np.stack([np.full(64, 8.0 * face_b), 8 * k[1] + rng.uniform(0, 8, 64), 8 * k[2] + rng.uniform(0, 8, 64)], axis=1) for k in cut])
    lo, hi = idx.keys.min(axis=0) * 8.0, (idx.keys.max(axis=0) + 1) * 8.0
    pts = np.concatenate([centres, on_face, rng.uniform(lo, hi, (4096, 3))])
    pose = G.pose_of(ctx)
    co, cd = camera_rays(pose, G.CAM, cell, o)
    near, far = f32(S.STOCK["depth_trunc_min"]) / cell, f32(S.STOCK["depth_trunc_max"]) / cell
    beyond = np.array([k for k in held if k not in window and k[0] >= face_b], np.float64)
    assert len(beyond) >= 8
    so = beyond[rng.integers(0, len(beyond), 512)] * 8 + rng.uniform(0, 8, (512, 3))
    st = o + rng.uniform(8, res - 8, (512, 3))
    sd = st - so
    ln = np.linalg.norm(sd, axis=1)
    rays = (np.concatenate([co, so]), np.concatenate([cd, (sd / ln[:, None]).astype(f32)]),
            np.concatenate([np.full(len(co), near, f32), np.zeros(512, f32)]), np.concatenate([np.full(len(co), far, f32), ln.astype(f32)]))
    return pts, rays, f32(0.7 * 5)                                # the raycaster's increment, 0.7 of the truncation of 5 cells, in voxels


def check_mixed(ctx, color, store=True):
    """the queries run FIRST (the read-outs that build the dictionary settle pending weights); returns what the caller may want to look at"""
    o = ctx.volume_origin()
    assert o == SHIFT
    # a first dictionary only to place the queries: read-outs do not change what the map is
    probe, window = map_dict(ctx, color, store)
    idx = E.MapIndex(probe)
    pts, rays, step = mixed_queries(ctx, window, idx) if store else (None, None, None)
    return probe, window, idx, pts, rays, step


@pytest.mark.parametrize("res,color", CASES)
def test_mixed_sources(res, color):
    ctx = mixed_ctx(res, color)
    d, window, idx, pts, rays, step = check_mixed(ctx, color)
    want = E.np_sample(idx, pts, detail=True)
    is_win = np.array([tuple(k) in window for k in idx.keys.tolist()] + [False])
    sl = want["slots"]
    both = want["observed"] & np.any(is_win[sl], axis=1) & np.any(~is_win[sl] & (sl >= 0), axis=1)
    print(res, color, "points", len(pts), "observed", int(np.count_nonzero(want["observed"])), "observed with corners from window and store", int(np.count_nonzero(both)))
    assert np.count_nonzero(both) >= 256 and np.count_nonzero(want["observed"]) >= 512
    assert_same(ctx.map_sample(pts), want, SAMPLE_KEYS, "mixed points")
    want_r = E.np_cast(idx, *rays, step)
    n_cam = len(rays[0]) - 512
    print("camera rays hit", int(np.count_nonzero(want_r["status"][:n_cam] == E.HIT)), "of", n_cam, "store-to-window rays hit", int(np.count_nonzero(want_r["status"][n_cam:] == E.HIT)))
    assert np.count_nonzero(want_r["status"][:n_cam] == E.HIT) >= n_cam // 4 and np.count_nonzero(want_r["status"][n_cam:] == E.HIT) >= 8
    assert_same(ctx.map_cast_rays(*rays, step), want_r, CAST_KEYS, "mixed rays")
    ctx.close()


def fuse_on(ctx, frames):
    """further frames fused at their true poses in the shifted window, without tracking: with set_defer(1) their free-space weights stay pending in the words"""
    size, res = ctx.size, ctx.res
    cell = f32(size) / f32(res)
    for k in frames:
        ctx.upload_depth_mm(G.frame(k, size))
        ctx.preprocess(G.P["depth_trunc_min"], G.P["depth_trunc_max"], G.P["filter_sigma_pixel"], G.P["filter_sigma_depth"])
        ctx.integrate(G.moved_pose(S.trajectory_pose(k, size).astype(f32), SHIFT, cell), 5 * size / res, G.GATE)


@pytest.mark.parametrize("max_weight", [2.0, 128.0])
def test_deferred_weights(max_weight):
    """set_defer(1): the window's stored weights lag behind, the deferred-weight words carry the rest (max_weight 2: saturated quarters, KF_PEND_SAT).  The
    queries run while the words are live -- nothing has read the volume out since the last deferred fusion pass -- and must report the TRUE weights, those
    of the read-out taken afterwards"""
    res = 64
    ctx = mixed_ctx(res, False, defer=1, max_weight=max_weight)
    _, window, idx0, pts, rays, step = check_mixed(ctx, False)
    fuse_on(ctx, (6, 7, 8))
    assert ctx.fusion_form()["defer"] == 1
    got_s, got_r = ctx.map_sample(pts), ctx.map_cast_rays(*rays, step)
    d, _ = map_dict(ctx, False)                                   # (after the queries)
    idx = E.MapIndex(d)
    want = E.np_sample(idx, pts)
    if max_weight == 2.0:
        assert np.count_nonzero(want["weight"] == f32(max_weight)) >= 256                     # saturated
    else:
        assert np.count_nonzero(want["weight"] != E.np_sample(idx0, pts)["weight"]) >= 256   # the three frames did move weights
    assert_same(got_s, want, SAMPLE_KEYS, "deferred points")
    assert_same(got_r, E.np_cast(idx, *rays, step), CAST_KEYS, "deferred rays")
    ctx.close()


def test_no_store_reserved():
    """the window alone is the map; everything outside it reads unobserved"""
    res = 64
    ctx = mixed_ctx(res, False, store=False)
    d, window = map_dict(ctx, False, store=False)
    idx = E.MapIndex(d)
    rng = np.random.default_rng(43)
    o = np.array(ctx.volume_origin(), np.float64)
    seen = np.argwhere(G.planes(ctx)[1] > 0)[:, ::-1]             # observed voxels of the window, (x, y, z)
    near = o + seen[rng.integers(0, len(seen), 2048)] + rng.uniform(0, 1, (2048, 3))
    pts = np.concatenate([o + rng.uniform(-16, res + 16, (4096, 3)), near])
    want = E.np_sample(idx, pts)
    outside = np.any((pts < o + 0.5) | (pts > o + res - 0.5), axis=1)
    assert np.count_nonzero(outside) >= 1024 and not want["observed"][outside].any() and np.count_nonzero(want["observed"]) >= 512
    assert_same(ctx.map_sample(pts), want, SAMPLE_KEYS, "no store")
    co, cd = camera_rays(G.pose_of(ctx), G.CAM, f32(ctx.size) / f32(res), ctx.volume_origin())
    want_r = E.np_cast(idx, co, cd, f32(6), f32(96), 3.5)
    assert np.count_nonzero(want_r["status"] == E.HIT) >= 256
    assert_same(ctx.map_cast_rays(co, cd, f32(6), f32(96), 3.5), want_r, CAST_KEYS, "no store, rays")
    ctx.close()


# ---- 3. device and host forms, NULL outputs, refusals ------------------------------------------------------------------------------------------------
def test_device_form_and_null_outputs():
    import torch
    color = True
    ctx = store_only_ctx(64, color, E.sphere_map())
    want_s, want_r = sphere_expected(color)
    pts, (o, d, t0, t1) = E.sphere_points(), E.sphere_rays()
    n, m = len(pts), len(o)
    dev = torch.device("cuda")
    d_pos = torch.from_numpy(pts).to(dev)
    out = dict(tsdf=torch.full((n,), 7.0, device=dev), weight=torch.full((n,), 7.0, device=dev), grad=torch.full((n, 3), 7.0, device=dev),
               color=torch.full((n, 4), 7, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    ctx.map_sample_device(n, d_pos.data_ptr(), out["tsdf"].data_ptr(), out["weight"].data_ptr(), out["grad"].data_ptr(), out["color"].data_ptr())
    ctx.sync()
    assert_same({k: v.cpu().numpy() for k, v in out.items()}, want_s, SAMPLE_KEYS, "device points")
    for keep in SAMPLE_KEYS:                                      # one output at a time, the others NULL and untouched
        for v in out.values():
            v.fill_(7)
        torch.cuda.synchronize()
        ctx.map_sample_device(n, d_pos.data_ptr(), **{"dev_" + keep: out[keep].data_ptr()})
        ctx.sync()
        for k, v in out.items():
            if k == keep:
                assert np.array_equal(bits(v.cpu().numpy()), bits(want_s[k])), keep
            else:
                assert bool((v == 7).all()), (keep, k)
        assert_same(ctx.map_sample(pts, want=(keep,)), want_s, (keep,), "host points, one output")
    d_o, d_d, d_t0, d_t1 = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (o, d, t0, t1))
    rout = dict(status=torch.full((m,), 7, dtype=torch.uint8, device=dev), t=torch.full((m,), 7.0, device=dev), normal=torch.full((m, 3), 7.0, device=dev),
                color=torch.full((m, 4), 7, dtype=torch.uint8, device=dev), weight=torch.full((m,), 7.0, device=dev))
    torch.cuda.synchronize()
    ctx.map_cast_rays_device(m, d_o.data_ptr(), d_d.data_ptr(), d_t0.data_ptr(), d_t1.data_ptr(), E.STEP, 1 << 24, *[rout[k].data_ptr() for k in CAST_KEYS])
    ctx.sync()
    assert_same({k: v.cpu().numpy() for k, v in rout.items()}, want_r, CAST_KEYS, "device rays")
    for keep in CAST_KEYS:
        for v in rout.values():
            v.fill_(7)
        torch.cuda.synchronize()
        ctx.map_cast_rays_device(m, d_o.data_ptr(), d_d.data_ptr(), d_t0.data_ptr(), d_t1.data_ptr(), E.STEP, 1 << 24, **{"dev_" + keep: rout[keep].data_ptr()})
        ctx.sync()
        for k, v in rout.items():
            if k == keep:
                assert np.array_equal(bits(v.cpu().numpy()), bits(want_r[k])), keep
            else:
                assert bool((v == 7).all()), (keep, k)
        assert_same(ctx.map_cast_rays(o, d, t0, t1, E.STEP, want=(keep,)), want_r, (keep,), "host rays, one output")
    # max_steps cuts the march where the restatement cuts it
    for steps in (1, 30):
        assert_same(ctx.map_cast_rays(o, d, t0, t1, E.STEP, max_steps=steps), E.np_cast(strip_color(E.sphere_map(), color), o, d, t0, t1, E.STEP, max_steps=steps), CAST_KEYS, steps)
    ctx.close()


def test_refusals():
    lib = K.load()
    p = K._p
    ctx = store_only_ctx(64, False, E.plane_map())
    pos, d = np.full((4, 3), 30.5), np.ones((4, 3), f32)
    t0, t1 = np.zeros(4, f32), np.full(4, 9, f32)
    f4, f12, b4, b16 = np.full(4, 7, f32), np.full(12, 7, f32), np.full(4, 7, np.uint8), np.full(16, 7, np.uint8)

    def untouched():
        return (f4 == 7).all() and (f12 == 7).all() and (b4 == 7).all() and (b16 == 7).all()
    # n = 0 is fine and does nothing, whatever the pointers hold
    assert lib.kf_map_sample(ctx.h, 0, p(pos), p(f4), p(f4), p(f12), p(b16)) == 0 and lib.kf_map_sample_device(ctx.h, 0, p(pos), None, None, None, None) == 0
    assert lib.kf_map_cast_rays(ctx.h, 0, p(pos), p(d), p(t0), p(t1), 0.5, 10, p(b4), p(f4), p(f12), p(b16), p(f4)) == 0
    assert lib.kf_map_cast_rays_device(ctx.h, 0, p(pos), p(d), p(t0), p(t1), 0.5, 10, None, None, None, None, None) == 0
    assert lib.kf_map_sample(ctx.h, 4, None, p(f4), p(f4), p(f12), p(b16)) == ARG
    for fn in (lib.kf_map_cast_rays, lib.kf_map_cast_rays_device):
        for step, steps in ((0.0, 10), (-1.0, 10), (float("nan"), 10), (float("inf"), 10), (0.5, 0), (0.5, (1 << 24) + 1)):
            assert fn(ctx.h, 4, p(pos), p(d), p(t0), p(t1), step, steps, p(b4), p(f4), p(f12), p(b16), p(f4)) == ARG, (step, steps)
        assert fn(ctx.h, 4, p(pos), None, p(t0), p(t1), 0.5, 10, p(b4), p(f4), p(f12), p(b16), p(f4)) == ARG
    assert untouched()
    assert lib.kf_map_cast_rays(ctx.h, 4, p(pos), p(d), p(t0), p(t1), 0.5, 1 << 24, p(b4), p(f4), p(f12), p(b16), p(f4)) == 0 and not untouched()
    ctx.close()
    f4[:], f12[:], b4[:], b16[:] = 7, 7, 7, 7
    slab = K.Context(K.camera(*G.CAM), 64, 2.0, G.P["volume_max_weight"], levels=3, slab=(0, 32))
    assert lib.kf_map_sample(slab.h, 4, p(pos), p(f4), p(f4), p(f12), p(b16)) == STATE and lib.kf_map_sample_device(slab.h, 4, p(pos), None, None, None, None) == STATE
    for fn in (lib.kf_map_cast_rays, lib.kf_map_cast_rays_device):
        assert fn(slab.h, 4, p(pos), p(d), p(t0), p(t1), 0.5, 10, p(b4), p(f4), p(f12), p(b16), p(f4)) == STATE
    assert untouched()
    slab.close()


# ---- 4. bystander ------------------------------------------------------------------------------------------------------------------------------------
def digest(ctx, color):
    keys, t, w, c = B.store_sorted(ctx)
    maps = [ctx.download_map(i, lv) for i in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS) for lv in range(3)]
    return [bits(a).tobytes() for a in G.planes(ctx, color) if a is not None] + [bits(a).tobytes() for a in (keys, t, w) + ((c,) if c is not None else ())] + \
           [bits(G.pose_of(ctx)).tobytes(), repr(ctx.volume_origin()), repr(ctx.brick_store_count())] + [bits(a).tobytes() for a in maps]


@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_bystander(res, color):
    """a digest of volume, store, pose, model maps and counts is the same before and after both calls; and a context that queried BEFORE anything read the
    deferred-weight words out goes on exactly as its twin that never queried: the next frame's pose and volume are equal"""
    a, b = mixed_ctx(res, color, defer=1), mixed_ctx(res, color, defer=1)
    _, window, idx, pts, rays, step = check_mixed(b, color)       # placed on the twin: nothing has read A's volume out
    if not color:
        fuse_on(a, (6, 7))
        fuse_on(b, (6, 7))                                        # live words on both
    first = a.map_sample(pts), a.map_cast_rays(*rays, step)
    assert np.count_nonzero(first[0]["weight"]) >= 512 and np.count_nonzero(first[1]["status"] == K.RAY_HIT) >= 256
    before = digest(a, color)
    second = a.map_sample(pts), a.map_cast_rays(*rays, step)
    assert_same(second[0], first[0], SAMPLE_KEYS, "asked again")
    assert_same(second[1], first[1], CAST_KEYS, "asked again")
    assert digest(a, color) == before
    assert digest(b, color) == before
    for ctx in (a, b):                                            # the next frame, tracked or not: the same on both
        G.run_frame(ctx, 8, color)
    assert digest(a, color) == digest(b, color)
    a.close()
    b.close()


# ---- 5. through the application ----------------------------------------------------------------------------------------------------------------------
def test_application_in_metres():
    res, color = 64, False
    size, cam = G.SIZES[res], G.CAM
    cell = f32(size) / f32(res)
    trunc = f32(5 * size / res)
    app = M.make_app(res, size, cam, color)
    try:
        app.set_brick_store(CAP)
        for k in range(6):
            assert M.app_frame(app, k, size, cam, color), k
            if k == 2:
                assert app.shift_volume(32, 0, 0)
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), res, size)
        rng = np.random.default_rng(47)
        o = np.array(app.volume_origin(), np.float64)
        pts_m = (o + rng.uniform(-24, res, (4096, 3))) * float(cell)
        vox = pts_m / np.float64(cell)
        got, ref = app.sample_map(pts_m), ctx.map_sample(vox)
        assert np.count_nonzero(ref["weight"]) >= 128
        assert np.array_equal(bits(got["distance"]), bits(ref["tsdf"] * trunc)) and np.array_equal(bits(got["weight"]), bits(ref["weight"]))
        assert np.array_equal(bits(got["gradient"]), bits(ref["grad"] * trunc / cell)) and np.array_equal(got["color"], ref["color"])
        pose = app.pose()[1]
        co, cd = camera_rays(pose, cam, cell, o)
        t0_m, t1_m = np.full(len(co), 0.2, f32), np.full(len(co), 3.0, f32)
        got = app.cast_map_rays(co * float(cell), cd, t0_m, t1_m)
        inc = f32(0.7) * trunc                                    # the raycaster's increment (AppParams)
        ref = ctx.map_cast_rays((co * float(cell)) / np.float64(cell), cd, t0_m / cell, t1_m / cell, inc / cell)
        assert np.count_nonzero(ref["status"] == K.RAY_HIT) >= 512
        assert np.array_equal(got["status"], ref["status"]) and np.array_equal(bits(got["t"]), bits(ref["t"] * cell))
        for k in ("normal", "color", "weight"):
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
    finally:
        app.close()


def test_slab_application_refuses():
    sl = H.SlabsApp(64, 2.0, G.CAM, [0, 32, 64])
    try:
        with pytest.raises(K.KfError):
            sl.sample_map(np.zeros((2, 3)))
        with pytest.raises(K.KfError):
            sl.cast_map_rays(np.zeros((2, 3)), np.ones((2, 3), f32), 0.0, 1.0)
    finally:
        sl.close()
