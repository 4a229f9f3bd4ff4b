"""GPU: merging maps under a rigid transform.  kf_merge_brick_store_rigid resamples the incoming map at the destination's voxel centres -- trilinear in
tsdf and colour, the least weight of the used corners, unobserved where a used corner is -- and merges the result by kf_merge_brick_store's rule;
kf_rigid_brick_keys lists the destination bricks it looks at; HybKinectfu::mergeMap(path, Mat44) puts a map file behind both.

The yardstick is the numpy restatement of the rule (include/hybkf.h) below, np_resample: float64 for a brick's base corner, float32 arrays with one
rounded operation per operation for the rest, evaluated densely over the bounding box of everything the source can reach, widened by two bricks, WITHOUT the
candidate list; its result goes through test_gpu_map_merge.np_merge.  Shapes, sessions and helpers are those of test_gpu_map_merge.py (imported): 64 voxels
at 2.0 m with and without colour, 72 at 2.25 m, a store of 1024 bricks.  Everything is compared as integers, bit for bit, but for the geometry test, whose
tolerance is derived there."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_map_merge as MM
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
u32 = B.u32
CAP = B.CAP
CASES = B.CASES
ARG, STATE = 1001, 1002
np_merge, same_store, store_sorted, session_map, two_maps, keyset = MM.np_merge, M.same_store, B.store_sorted, MM.session_map, MM.two_maps, MM.keyset


def rotation(deg, axis):
    """Rodrigues, float64"""
    k = np.asarray(axis, f64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(a) * np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * np.outer(k, k)


def xf_of(r, t):
    return np.concatenate([np.asarray(r, f64), np.asarray(t, f64).reshape(3, 1)], axis=1)


GENERAL = xf_of(rotation(20, (1, 2, 3)), (2.3, -1.7, 0.4))
QUARTER_Z = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f64)     # x -> y, y -> -x
HALF_X = np.diag([1.0, -1.0, -1.0])


# ---- dense arrays ----------------------------------------------------------------------------------------------------------------------------------
def dense_of(m, pad=1):
    """map m as dense planes in (z, y, x) order over its keys' box, `pad` bricks wider on every side: (origin in voxels (x, y, z), tsdf, weight, colour);
    a brick the map does not hold reads as zeros"""
    lo, hi = m[0].min(axis=0) - pad, m[0].max(axis=0) + 1 + pad
    n = (hi - lo)[::-1] * 8                                       # (z, y, x)
    t, w = np.zeros(n, f32), np.zeros(n, f32)
    c = np.zeros(tuple(n) + (3,), np.uint8) if m[3] is not None else None
    for i, k in enumerate(m[0].tolist()):
        x, y, z = ((k[j] - lo[j]) * 8 for j in range(3))
        t[z:z + 8, y:y + 8, x:x + 8], w[z:z + 8, y:y + 8, x:x + 8] = m[1][i], m[2][i]
        if c is not None:
            c[z:z + 8, y:y + 8, x:x + 8] = m[3][i]
    return lo * 8, t, w, c


def rebrick(origin, t, w, c):
    """dense planes standing at `origin` (voxels, any integers) -> the sorted map of the bricks with a weight > 0; a voxel whose weight is not > 0 is
    unobserved: tsdf 0, weight 0, colour 0"""
    origin = np.asarray(origin, np.int64)
    o8 = (origin >> 3) << 3
    off = (origin - o8)[::-1]
    n = [int(-(-(s + o) // 8) * 8) for s, o in zip(t.shape[:3], off)]
    obs = w > 0
    T, W = np.zeros(n, f32), np.zeros(n, f32)
    sl = tuple(slice(int(o), int(o) + s) for o, s in zip(off, t.shape[:3]))
    T[sl], W[sl] = np.where(obs, t, f32(0)), np.where(obs, w, f32(0))
    Cc = None
    if c is not None:
        Cc = np.zeros(n + [3], np.uint8)
        Cc[sl] = np.where(obs[..., None], c, np.uint8(0))
    keys, bt, bw, bc = [], [], [], []
    for z in range(0, n[0], 8):
        for y in range(0, n[1], 8):
            for x in range(0, n[2], 8):
                if np.any(W[z:z + 8, y:y + 8, x:x + 8] > 0):
                    keys.append((o8[0] // 8 + x // 8, o8[1] // 8 + y // 8, o8[2] // 8 + z // 8))
                    bt.append(T[z:z + 8, y:y + 8, x:x + 8]); bw.append(W[z:z + 8, y:y + 8, x:x + 8])
                    if c is not None:
                        bc.append(Cc[z:z + 8, y:y + 8, x:x + 8])
    return np.array(keys, np.int32).reshape(-1, 3), np.stack(bt), np.stack(bw), np.stack(bc) if c is not None else None


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------------------
def np_resample(m, xf):
    """the rule of kf_merge_brick_store_rigid, densely: -> (the resampled map: every brick of the box, sorted (z, y, x), also those without a weight;
    mixed: per brick the number of voxels dropped because a used corner is unobserved while another used one is observed)"""
    xf = np.asarray(xf, f64)
    r, t = xf[:, :3], xf[:, 3]
    color = m[3] is not None
    so, st, sw, sc = dense_of(m, pad=1)
    # the box of destination bricks: the source's box (with its +-1 voxel reach) transformed in float64, widened by two bricks
    lo, hi = m[0].min(axis=0) * 8.0 - 1.0, (m[0].max(axis=0) + 1) * 8.0
    cs = np.array([[(hi if (c >> j) & 1 else lo)[j] + 0.5 for j in range(3)] for c in range(8)])
    d = cs @ r.T + t - 0.5
    b0, b1 = (np.floor(d.min(axis=0)).astype(np.int64) >> 3) - 2, (np.ceil(d.max(axis=0)).astype(np.int64) >> 3) + 2
    kz, ky, kx = np.meshgrid(np.arange(b0[2], b1[2] + 1), np.arange(b0[1], b1[1] + 1), np.arange(b0[0], b1[0] + 1), indexing="ij")
    keys = np.stack([kx, ky, kz], -1).reshape(-1, 3)              # (z, y, x) order
    # per brick, float64:  a = 8 K + 0.5 - t;  c_j = ((R[0][j] a_0 + R[1][j] a_1) + R[2][j] a_2) - 0.5
    a = 8.0 * keys.astype(f64) + 0.5 - t
    ib, fb = np.empty((len(keys), 3), np.int64), np.empty((len(keys), 3), f32)
    for j in range(3):
        c = ((r[0, j] * a[:, 0] + r[1, j] * a[:, 1]) + r[2, j] * a[:, 2]) - 0.5
        fl = np.floor(c)
        frac = (c - fl).astype(f32)
        up = frac == f32(1)
        ib[:, j], fb[:, j] = fl.astype(np.int64) + up, np.where(up, f32(0), frac)
    # per voxel, float32:  u_j = ((Rf[0][j] lx + Rf[1][j] ly) + Rf[2][j] lz) + fb_j
    rf = r.astype(f32)
    lz, ly, lx = (v.astype(f32)[None] for v in np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"))
    i, f = [], []
    for j in range(3):
        u = ((rf[0, j] * lx + rf[1, j] * ly) + rf[2, j] * lz) + fb[:, j, None, None, None]
        assert u.dtype == f32
        n = np.floor(u)
        f.append(u - n)
        i.append(ib[:, j, None, None, None] + n.astype(np.int64))
    assert f[0].dtype == f32
    # the eight corners
    shape = np.array(st.shape)                                    # (z, y, x)
    ct, cw, cc, used, seen = [], [], [], [], []
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        us = ((f[0] > 0) | (dx == 0)) & ((f[1] > 0) | (dy == 0)) & ((f[2] > 0) | (dz == 0))
        x, y, z = i[0] + dx - so[0], i[1] + dy - so[1], i[2] + dz - so[2]
        inside = (x >= 0) & (x < shape[2]) & (y >= 0) & (y < shape[1]) & (z >= 0) & (z < shape[0])
        x, y, z = np.clip(x, 0, shape[2] - 1), np.clip(y, 0, shape[1] - 1), np.clip(z, 0, shape[0] - 1)
        w = np.where(inside, sw[z, y, x], f32(0))
        ct.append(st[z, y, x]); cw.append(w); used.append(us); seen.append(w > 0)
        if color:
            cc.append(sc[z, y, x].astype(f32))
    bad = np.zeros(f[0].shape, bool)
    some = np.zeros(f[0].shape, bool)
    wmin = np.full(f[0].shape, np.inf, f32)
    for k in range(8):
        bad |= used[k] & ~seen[k]
        some |= used[k] & seen[k]
        wmin = np.where(used[k], np.minimum(wmin, cw[k]), wmin)
    ok = ~bad

    def lerps(v, fs):
        """v: the 8 corner arrays (..., [3]); x, then y, then z; an axis with f == 0 passes its value on"""
        ex = (lambda q: q[..., None]) if v[0].ndim == 5 else (lambda q: q)
        v = [np.where(ex(fs[0] > 0), v[k] + ex(fs[0]) * (v[k + 1] - v[k]), v[k]) for k in (0, 2, 4, 6)]
        v = [np.where(ex(fs[1] > 0), v[k] + ex(fs[1]) * (v[k + 1] - v[k]), v[k]) for k in (0, 2)]
        out = np.where(ex(fs[2] > 0), v[0] + ex(fs[2]) * (v[1] - v[0]), v[0])
        assert out.dtype == f32
        return out

    rt = np.where(ok, lerps(ct, f), f32(0))
    rw = np.where(ok, wmin, f32(0)).astype(f32)
    rc = None
    if color:
        rc = np.where(ok[..., None], np.minimum(f32(255), lerps(cc, f) + f32(0.5)).astype(np.uint8), np.uint8(0))
    mixed = np.count_nonzero(bad & some, axis=(1, 2, 3))
    return (keys.astype(np.int32), rt, rw, rc), mixed


def observed(b):
    """the bricks of a resampled map with a weight > 0"""
    keep = np.any(b[2] > 0, axis=(1, 2, 3))
    return b[0][keep], b[1][keep], b[2][keep], b[3][keep] if b[3] is not None else None


_RESAMPLED = {}


def resampled(res, color, which, name, xf):
    """computed once per shape and shared; nobody writes into the arrays"""
    key = (res, color, which, name)
    if key not in _RESAMPLED:
        _RESAMPLED[key] = np_resample(session_map(res, color, which), xf)
    return _RESAMPLED[key]


def rigid_raw(ctx, n, keys, t, w, c, xf):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return ctx.lib.kf_merge_brick_store_rigid(ctx.h, n, p(keys), p(t), p(w), p(c), K.rigid_xf(xf) if xf is not None else None)


# ---- 1. identity and brick translations: kf_merge_brick_store -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_identity_and_whole_bricks_equal_the_plain_merge(res, color):
    a, b = two_maps(res, color)
    for t, off in (((0, 0, 0), None), ((8, -16, 24), (1, -2, 3))):
        m1, m2 = MM.store_ctx(res, color, a), MM.store_ctx(res, color, a)
        m1.merge_brick_store_rigid(b[0], b[1], b[2], b[3], xf_of(np.eye(3), t))
        m2.merge_brick_store(b[0], b[1], b[2], b[3], offset=off)
        got, want = store_sorted(m1), store_sorted(m2)
        assert same_store(got, want) and m1.brick_store_count() == m2.brick_store_count() and m1.brick_store_count()[1] == 0, t
        m1.close(); m2.close()


def pending_store(res=64, maxw=MM.MAXW):
    """test_gpu_map_merge.test_held_slots_with_a_pending_word's store: fused with deferral forced on, its bricks gone by a shift with their deferred-weight
    words.  Returns the context and its read-out (true weights)."""
    a = K.Context(K.camera(*G.CAM), res, G.SIZES[res], maxw, levels=3)
    a.set_defer(1)
    a.brick_store_reserve(CAP)
    G.fuse(a, range(6))
    assert a.fusion_form()["defer"] == 1
    a.shift_volume(0, -24, 16)
    before = store_sorted(a)
    assert len(before[0]) >= 20 and a.brick_store_count() == (len(before[0]), 0, 0)
    return a, before


def test_identity_onto_held_slots_with_a_pending_word():
    """the held path with deferred-weight words not 0: the rigid merge starts from the TRUE weights and leaves words of 0, as the plain merge does"""
    _, b = two_maps(64, False)
    (m1, before), (m2, twin) = pending_store(), pending_store()
    assert same_store(before, twin) and keyset(before) & keyset(b)
    m1.merge_brick_store_rigid(b[0], b[1], b[2], None, xf_of(np.eye(3), (0, 0, 0)))
    m2.merge_brick_store(b[0], b[1], b[2])
    first = store_sorted(m1)
    assert same_store(first, store_sorted(m2)) and same_store(first, np_merge(before, b)) and not same_store(first, before)
    assert m1.brick_store_count() == m2.brick_store_count() and m1.brick_store_count()[1] == 0
    assert same_store(store_sorted(m1), first)                    # a second read-out applies nothing twice
    m1.close(); m2.close()


# ---- 2. whole voxels, not whole bricks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_whole_voxels_are_a_verbatim_copy(res, color):
    a, _ = two_maps(res, color)
    t = (3, -5, 12)
    o, dt, dw, dc = dense_of(a, pad=0)
    want = rebrick(o + np.array(t), dt, dw, dc)                   # the dense source rolled by t, bricked again
    assert len(want[0]) > len(a[0]) // 2
    ctx = MM.store_ctx(res, color)
    ctx.merge_brick_store_rigid(a[0], a[1], a[2], a[3], xf_of(np.eye(3), t))
    assert same_store(store_sorted(ctx), want) and ctx.brick_store_count() == (len(want[0]), 0, 0)
    ctx.close()


# ---- 3. signed permutations ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_signed_permutations_reindex_exactly(res, color):
    """d = R (s + 1/2) + t - 1/2.  A quarter turn about z: dx = -sy + tx - 1, dy = sx + ty, dz = sz + tz; a half turn about x: dx = sx + tx,
    dy = -sy + ty - 1, dz = -sz + tz - 1.  On planes in (z, y, x) order that is np.rot90 in the (x, y) plane and a flip of y and z."""
    a, _ = two_maps(res, color)
    o, dt, dw, dc = dense_of(a, pad=0)
    nz, ny, nx = dt.shape
    t = np.array((3, -5, 12))
    turned = lambda p: np.rot90(p, 1, axes=(2, 1))                # out[z, sx, ny - 1 - sy] = p[z, sy, sx]
    origin_q = np.array([-(o[1] + ny - 1) + t[0] - 1, o[0] + t[1], o[2] + t[2]])
    flipped = lambda p: np.flip(p, axis=(0, 1))
    origin_h = np.array([o[0] + t[0], -(o[1] + ny - 1) + t[1] - 1, -(o[2] + nz - 1) + t[2] - 1])
    for r, fn, origin in ((QUARTER_Z, turned, origin_q), (HALF_X, flipped, origin_h)):
        want = rebrick(origin, fn(dt), fn(dw), fn(dc) if color else None)
        ctx = MM.store_ctx(res, color)
        ctx.merge_brick_store_rigid(a[0], a[1], a[2], a[3], xf_of(r, t))
        assert same_store(store_sorted(ctx), want) and ctx.brick_store_count() == (len(want[0]), 0, 0), r
        ctx.close()


# ---- 4. a general transform against numpy; 5. the candidates are complete ---------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
@pytest.mark.parametrize("held,incoming", [("A", "B"), ("B", "A")])
def test_general_transform_against_numpy(res, color, held, incoming):
    two_maps(res, color)
    a, b = session_map(res, color, held), session_map(res, color, incoming)
    rb, mixed = resampled(res, color, incoming, "general", GENERAL)
    ob = observed(rb)
    cand = keyset((K.rigid_brick_keys(b[0], GENERAL),))
    ia = {tuple(k): i for i, k in enumerate(a[0].tolist())}
    blended = sum(int(np.count_nonzero((a[2][ia[tuple(k)]] > 0) & (ob[2][i] > 0))) for i, k in enumerate(ob[0].tolist()) if tuple(k) in ia)
    fresh = keyset(ob) - keyset(a)
    idle = cand - keyset(ob)
    print(res, color, held, "<-", incoming, "resampled bricks", len(ob[0]), "candidates", len(cand), "blended voxels", blended, "fresh bricks", len(fresh),
          "candidates without a slot", len(idle), "voxels with observed and unobserved corners", int(mixed.sum()))
    assert blended >= 1000 and len(fresh) >= 1 and len(idle) >= 1 and mixed.sum() >= 100
    assert keyset(ob) <= cand                                      # 5. every brick the dense evaluation gives a weight is a candidate
    want = np_merge(a, ob)
    ctx = MM.store_ctx(res, color, a)
    ctx.merge_brick_store_rigid(b[0], b[1], b[2], b[3], GENERAL)
    got = store_sorted(ctx)
    assert np.array_equal(got[0], want[0])
    assert same_store(got, want) and ctx.brick_store_count() == (len(want[0]), 0, 0)
    ctx.close()


# ---- 6. geometry, independent of the restatement ------------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.48, -0.6, 0.64])                            # |n| = 1
PLANE_H, PLANE_TRUNC, PLANE_NB = 14.0, 12.0, 6


def plane_map():
    """the truncated SDF of the plane n . x = h (x: voxel centres, in voxels), all weights 1, 6^3 bricks from key (0, 0, 0) on"""
    n = PLANE_NB * 8
    z, y, x = np.meshgrid(*(np.arange(n) + 0.5,) * 3, indexing="ij")
    sdf = (PLANE_N[0] * x + PLANE_N[1] * y + PLANE_N[2] * z - PLANE_H) / PLANE_TRUNC
    t = np.clip(sdf, -1.0, 1.0).astype(f32)
    bz, by, bx = np.meshgrid(*(np.arange(PLANE_NB),) * 3, indexing="ij")
    keys = np.stack([bx, by, bz], -1).reshape(-1, 3).astype(np.int32)
    tb = np.ascontiguousarray(B.bricks(t).reshape(-1, 8, 8, 8))
    return (keys, tb, np.ones_like(tb), None)


def plane_expectation(keys):
    """for the destination bricks `keys`: the analytic SDF at every voxel centre carried back into the source (float64), and which voxels have all eight
    source corners inside the map and unclamped"""
    r, t = GENERAL[:, :3], GENERAL[:, 3]
    lz, ly, lx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    d = np.stack([keys[:, 0, None, None, None] * 8 + lx, keys[:, 1, None, None, None] * 8 + ly, keys[:, 2, None, None, None] * 8 + lz], -1).astype(f64)
    p = (d + 0.5 - t) @ r                                         # R^T (d + 1/2 - t): the centre's position in the source
    want = (p @ PLANE_N - PLANE_H) / PLANE_TRUNC
    base = np.floor(p - 0.5)
    good = np.ones(want.shape, bool)
    for k in range(8):
        c = base + np.array([k & 1, (k >> 1) & 1, k >> 2])
        v = ((c + 0.5) @ PLANE_N - PLANE_H) / PLANE_TRUNC
        good &= np.all((c >= 0) & (c < PLANE_NB * 8), axis=-1) & (np.abs(v) < 0.999)
    return want, good


def test_plane_count_needs_no_device():
    keys = K.rigid_brick_keys(plane_map()[0], GENERAL)
    assert np.count_nonzero(plane_expectation(keys)[1]) >= 2000


def test_geometry_of_a_resampled_plane():
    """A linear field is reproduced by trilinear interpolation up to rounding: seven lerps of values <= 1 and a position error below 4e-6 voxels (a slope of
    1 / 12 per voxel) stay under 3e-6, the source values' own fp32 rounding (6e-8) included; the bound asked is 1e-5 absolute.  A transposed rotation or a
    missing half voxel, which a restatement could share with the kernel, moves the plane by tenths."""
    src = plane_map()
    ctx = MM.store_ctx(64, False, cap=2048)
    ctx.merge_brick_store_rigid(src[0], src[1], src[2], None, GENERAL)
    got = store_sorted(ctx)
    ctx.close()
    want, good = plane_expectation(got[0].astype(np.int64))
    assert np.count_nonzero(good) >= 2000
    cand = K.rigid_brick_keys(src[0], GENERAL)
    assert np.count_nonzero(plane_expectation(cand.astype(np.int64))[1]) == np.count_nonzero(good)       # no such voxel lies in a brick that was not stored
    assert np.all(got[2][good] == 1)                              # observed, with the least weight of eight ones
    err = np.abs(got[1][good].astype(f64) - want[good])
    print("plane: voxels compared", np.count_nonzero(good), "max error", err.max())
    assert err.max() <= 1e-5


# ---- 7. bystanders and refusals --------------------------------------------------------------------------------------------------------------------------------
def test_bystanders_are_untouched():
    res, color = 64, False
    _, b = two_maps(res, color)
    ctx = MM.session(res, color, "A")
    ctx.brick_store_capture()
    G.raycast(ctx, color)
    maps = lambda: [ctx.download_map(m).copy() for m in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS)]
    planes, pose, origin, model = M.planes_bits(ctx, color), G.pose_of(ctx), ctx.volume_origin(), maps()
    before = store_sorted(ctx)
    ctx.merge_brick_store_rigid(b[0], b[1], b[2], None, GENERAL)
    assert not same_store(store_sorted(ctx), before)              # the store did change
    assert M.equal_bits(M.planes_bits(ctx, color), planes) and np.array_equal(u32(G.pose_of(ctx)), u32(pose)) and ctx.volume_origin() == origin
    assert all(G.same_bits(x, y) for x, y in zip(maps(), model))
    ctx.close()


def test_a_full_store_drops_and_keeps_held_keys_complete():
    res, color = 64, False
    a, b = two_maps(res, color)
    ob = observed(resampled(res, color, "B", "general", GENERAL)[0])
    want = np_merge(a, ob)
    new = len(want[0]) - len(a[0])
    assert new >= 2
    cap = len(a[0]) + new // 2                                    # room for half of what the merge adds
    ctx = MM.store_ctx(res, color, a, cap=cap)
    ctx.merge_brick_store_rigid(b[0], b[1], b[2], None, GENERAL)
    assert ctx.brick_store_count() == (cap, new - new // 2, 0)
    got = store_sorted(ctx)
    at = {tuple(k): i for i, k in enumerate(want[0].tolist())}
    assert keyset(a) <= keyset(got) <= keyset(want)
    for i, k in enumerate(got[0].tolist()):                       # every held key holds what the full merge gives it
        j = at[tuple(k)]
        assert np.array_equal(u32(got[1][i]), u32(want[1][j])) and np.array_equal(u32(got[2][i]), u32(want[2][j])), k
    ctx.close()


def test_refusals_touch_nothing():
    res = 64
    a, b = two_maps(res, False)
    ctx = MM.store_ctx(res, False, a)
    store, counts = store_sorted(ctx), ctx.brick_store_count()
    k2, t2, w2 = np.ascontiguousarray(b[0][:2]), np.ascontiguousarray(b[1][:2]), np.ascontiguousarray(b[2][:2])
    twice = np.ascontiguousarray(np.stack([b[0][0], b[0][0]]))
    assert rigid_raw(ctx, 2, twice, t2, w2, None, GENERAL) == ARG                                          # a key twice in one call
    assert rigid_raw(ctx, 2, None, t2, w2, None, GENERAL) == ARG and rigid_raw(ctx, 2, k2, None, w2, None, GENERAL) == ARG
    assert rigid_raw(ctx, 2, k2, t2, None, None, GENERAL) == ARG and rigid_raw(ctx, 2, k2, t2, w2, None, None) == ARG
    scaled, mirror, nan = GENERAL.copy(), GENERAL.copy(), GENERAL.copy()
    scaled[:, :3] *= 1.001; mirror[0, :3] *= -1; nan[1, 3] = np.nan
    for bad in (scaled, mirror, nan):                             # no rigid transform
        assert rigid_raw(ctx, 2, k2, t2, w2, None, bad) == ARG
    far = np.ascontiguousarray(np.stack([b[0][0], np.array((1 << 20, 0, 0), np.int32)]))
    assert rigid_raw(ctx, 2, far, t2, w2, None, GENERAL) == ARG                                            # a source key out of range
    push = xf_of(GENERAL[:, :3], (8.0 * (1 << 20), 0, 0))
    assert rigid_raw(ctx, 2, k2, t2, w2, None, push) == ARG                                                # a key out of range after transforming
    assert rigid_raw(ctx, 2, k2, t2, w2, np.zeros((2, 512, 3), np.uint8), GENERAL) == STATE                # colour without a colour plane
    assert rigid_raw(ctx, 0, None, None, None, None, None) == 0                                            # nothing to merge: no array is looked at
    assert same_store(store_sorted(ctx), store) and ctx.brick_store_count() == counts
    ctx.close()
    bare = G.make_ctx(res)                                        # no store
    assert rigid_raw(bare, 2, k2, t2, w2, None, GENERAL) == STATE and bare.brick_store_count() == (0, 0, 0)
    bare.close()


# ---- 8. the host class ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_host_class_merges_under_a_transform(tmp_path, res, color):
    size = G.SIZES[res]
    cam = G.RGB_CAM if color else G.CAM
    fa, fb = str(tmp_path / "a.hkfmap"), str(tmp_path / "b.hkfmap")
    b = MM.app_session(res, size, cam, color, "B", CAP)
    try:
        assert b.save_map(fb)
    finally:
        b.close()
    # the matrix in metres, as poses are; in voxels (include/hybkf.h, hybkf_host.hpp): t_vox = (double)t_m / (double)cell, cell the fp32 quotient
    cell = f32(size) / f32(res)
    mat = np.eye(4, dtype=f32)
    mat[:3, :3] = GENERAL[:, :3].astype(f32)
    mat[:3, 3] = (GENERAL[:, 3] * float(cell)).astype(f32)
    xf = xf_of(mat[:3, :3].astype(f64), mat[:3, 3].astype(f64) / f64(cell))
    small = 128                                                   # room for A's own capture, not for held + the candidates: the store has to grow
    a = MM.app_session(res, size, cam, color, "A", small)
    twin = G.make_ctx(res, color, 300000)
    try:
        assert a.save_map(fa)                                     # (captures: the store now holds A's whole map, and so does the file)
        ma, mb = MM.records(fa, color)[0], MM.records(fb, color)[0]
        ca = K.Context.borrow(a.ctx_handle(), K.camera(*cam), res, size)
        ca.has_color = color                                      # (brick_store() reads the colour plane of a context that says it has one)
        origin = a.volume_origin()
        pose, frame_id = a.pose()[1].copy(), a.frame_id()
        # the twin: A's map in a store, the window placed where A's stands
        twin.brick_store_reserve(small)
        twin.write_brick_store(ma[0], ma[1], ma[2], ma[3])
        twin.place_window(*origin)
        assert M.same_planes(ca, twin, color)
        assert a.merge_map_rigid(fb, mat)
        # the C-ABI sequence: capture, grow to held + candidates, one merge, refill
        twin.brick_store_capture()
        held = twin.brick_store_count()[0]
        cand = len(K.rigid_brick_keys(mb[0], xf))
        print(res, color, "held", held, "candidates", cand, "capacity", small)
        assert held <= small < held + cand
        k, t, w, c = twin.brick_store()                           # read out, reserved larger, written back
        twin.brick_store_reserve(held + cand)
        twin.write_brick_store(k, t, w, c)
        twin.merge_brick_store_rigid(mb[0], mb[1], mb[2], mb[3], xf)
        twin.refill_window()
        got, want = store_sorted(ca), store_sorted(twin)
        assert len(want[0]) > len(ma[0]) and same_store(got, want)
        assert a.brick_store_count()[:2] == (len(want[0]), 0)
        assert M.same_planes(ca, twin, color)
        assert np.array_equal(u32(a.pose()[1]), u32(pose)) and a.frame_id() == frame_id and a.volume_origin() == origin
        # no rigid transform, a brick pushed out of the key range: refused with planes and store untouched
        planes = M.planes_bits(ca, color)
        scaled, far = mat.copy(), mat.copy()
        scaled[:3, :3] *= f32(1.001)
        far[0, 3] = f32(8.0 * (1 << 20) * float(cell))
        for bad in (scaled, far):
            assert not a.merge_map_rigid(fb, bad)
            assert M.equal_bits(M.planes_bits(ca, color), planes) and same_store(store_sorted(ca), got)
        assert M.app_frame(a, 6, size, cam, color)                # tracked against the merged model
    finally:
        a.close()
        twin.close()


def test_slab_application_refuses(tmp_path):
    sl = H.SlabsApp(64, 2.0, G.CAM, [0, 32, 64])
    try:
        assert sl.merge_map_rigid(str(tmp_path / "x.hkfmap"), np.eye(4, dtype=f32)) is False
    finally:
        sl.close()
