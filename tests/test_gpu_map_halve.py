"""GPU: halving a map's resolution.  kf_merge_brick_store_halved reads an incoming map at voxel size s, forms every coarse voxel (size 2 s) from its eight
children -- the mean tsdf of the observed ones in a fixed order of additions, their least weight, their mean colour, unobserved where none is observed -- and
merges the result by kf_merge_brick_store's rule; kf_halved_brick_keys lists the coarse bricks; HybKinectfu::loadMapCoarser and tools/map_lod.py put a map file
behind both.

The yardstick is the numpy restatement of the rule (include/hybkf.h) below, np_halve: float32 arrays and integers, one rounded operation per operation, in the
order written there; its result goes through test_gpu_map_merge.np_merge.  Sessions and helpers are those of test_gpu_map_merge.py, test_gpu_map_file.py and
test_gpu_brickstore.py (imported).  The destination is a resolution-64 context with a reserved store: the raw entry never looks at the resolution.  Everything
is compared as integers, bit for bit."""
import ctypes as C
import importlib.util
import os
import struct

import numpy as np
import pytest

import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_map_merge as MM
import test_gpu_map_resample as R
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
u32 = B.u32
CAP = B.CAP
ARG, STATE = 1001, 1002
MAXW = MM.MAXW
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
np_merge, same_store, store_sorted, two_maps, keyset = MM.np_merge, M.same_store, B.store_sorted, MM.two_maps, MM.keyset
COLORS = [False, True]


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------------------
def child(a, i):
    """child i = dx | dy << 1 | dz << 2 of every coarse voxel of a (16, 16, 16[, 3]) block in (z, y, x) order -> (8, 8, 8[, 3])"""
    dx, dy, dz = i & 1, (i >> 1) & 1, i >> 2
    return a.reshape((8, 2, 8, 2, 8, 2) + a.shape[3:])[:, dz, :, dy, :, dx]


def np_halve(m, counts=None):
    """the rule of kf_merge_brick_store_halved: map m (keys, tsdf, weight, colour or None) -> the sorted map of the coarse bricks with a weight > 0.
    counts: a list of 9 zeros that takes the number of coarse voxels per number of observed children"""
    color = m[3] is not None
    at = {tuple(k): i for i, k in enumerate(m[0].tolist())}
    ck = np.unique(m[0].astype(np.int64) >> 1, axis=0)
    ck = ck[np.lexsort((ck[:, 0], ck[:, 1], ck[:, 2]))]
    keys, bt, bw, bc = [], [], [], []
    for kc in ck.tolist():
        t, w = np.zeros((16, 16, 16), f32), np.zeros((16, 16, 16), f32)
        c = np.zeros((16, 16, 16, 3), np.uint8)
        for d in range(8):
            dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
            i = at.get((2 * kc[0] + dx, 2 * kc[1] + dy, 2 * kc[2] + dz))
            if i is None:
                continue                                          # a brick the source does not hold: its voxels are unobserved
            sl = (slice(8 * dz, 8 * dz + 8), slice(8 * dy, 8 * dy + 8), slice(8 * dx, 8 * dx + 8))
            t[sl], w[sl] = m[1][i], m[2][i]
            if color:
                c[sl] = m[3][i]
        obs = w > 0
        cs = [child(np.where(obs, t, f32(0)), i) for i in range(8)]
        s = ((cs[0] + cs[1]) + (cs[2] + cs[3])) + ((cs[4] + cs[5]) + (cs[6] + cs[7]))
        n = sum(child(obs, i).astype(np.int64) for i in range(8))
        some = n > 0
        ht = np.where(some, s / np.maximum(n, 1).astype(f32), f32(0))
        wm = np.full((8, 8, 8), np.inf, f32)
        for i in range(8):
            wm = np.where(child(obs, i), np.minimum(wm, child(w, i)), wm)
        hw = np.where(some, wm, f32(0))
        assert s.dtype == f32 and ht.dtype == f32 and hw.dtype == f32
        if counts is not None:
            for k in range(9):
                counts[k] += int(np.count_nonzero(n == k))
        if not np.any(hw > 0):
            continue                                              # halves to nothing: takes no slot
        keys.append(kc); bt.append(ht); bw.append(hw)
        if color:
            tot = sum(child(np.where(obs[..., None], c, np.uint8(0)), i).astype(np.int64) for i in range(8))
            n3 = n[..., None]
            bc.append(np.where(some[..., None], (2 * tot + n3) // (2 * np.maximum(n3, 1)), 0).astype(np.uint8))
    if not keys:
        return (np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), f32), np.zeros((0, 8, 8, 8), f32), np.zeros((0, 8, 8, 8, 3), np.uint8) if color else None)
    return np.array(keys, np.int32).reshape(-1, 3), np.stack(bt), np.stack(bw), np.stack(bc) if color else None


def halved_raw(ctx, n, keys, t, w, c):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return ctx.lib.kf_merge_brick_store_halved(ctx.h, n, p(keys), p(t), p(w), p(c))


def sort_map(m):
    o = np.lexsort((m[0][:, 0], m[0][:, 1], m[0][:, 2]))
    return tuple(np.ascontiguousarray(x[o]) if x is not None else None for x in m)


def random_bricks(rng, keys, color, p_observed=0.5):
    """random weights in [1, max_weight] on a voxel observed with probability p_observed, random tsdf in (-1, 1] with some -0.0, random colours"""
    n = len(keys)
    w = np.where(rng.random((n, 8, 8, 8)) < p_observed, rng.integers(1, int(MAXW) + 1, (n, 8, 8, 8)), 0).astype(f32)
    t = (1.0 - 2.0 * rng.random((n, 8, 8, 8))).astype(f32)
    t[rng.random((n, 8, 8, 8)) < 0.02] = f32(-0.0)
    c = rng.integers(0, 256, (n, 8, 8, 8, 3), dtype=np.uint8) if color else None
    return np.ascontiguousarray(np.asarray(keys, np.int32).reshape(-1, 3)), t, w, c


def halved_into_empty(m, color, cap=CAP):
    ctx = MM.store_ctx(64, color, cap=cap)
    ctx.merge_brick_store_halved(m[0], m[1], m[2], m[3])
    got, counts = store_sorted(ctx), ctx.brick_store_count()
    ctx.close()
    return got, counts


# ---- 1. one fine brick: one octant of one coarse brick ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", COLORS)
def test_one_fine_brick_fills_one_octant(color):
    m = random_bricks(np.random.default_rng(3), [(-3, 1, -1)], color, p_observed=1.0)
    assert np.all(m[2] > 0)
    got, counts = halved_into_empty(m, color)
    assert counts == (1, 0, 0) and got[0].tolist() == [[-2, 0, -1]]          # -3 = 2 * -2 + 1, 1 = 2 * 0 + 1, -1 = 2 * -1 + 1: the octant (1, 1, 1)
    inside = np.zeros((8, 8, 8), bool)
    inside[4:, 4:, 4:] = True
    assert np.array_equal(got[2][0] > 0, inside)
    assert np.all(u32(got[1][0])[~inside] == 0) and np.all(u32(got[2][0])[~inside] == 0) and (not color or np.all(got[3][0][~inside] == 0))
    assert same_store(got, np_halve(m))


# ---- 2. eight full fine bricks: one full coarse brick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", COLORS)
def test_eight_full_bricks_give_one_full_brick(color):
    kc = np.array((3, -2, 1))
    keys = [tuple(2 * kc + np.array((d & 1, (d >> 1) & 1, d >> 2))) for d in range(8)]
    m = random_bricks(np.random.default_rng(4), keys, color, p_observed=1.0)
    got, counts = halved_into_empty(m, color)
    assert counts == (1, 0, 0) and got[0].tolist() == [kc.tolist()] and np.all(got[2] > 0)
    assert same_store(got, np_halve(m))
    for v in (f32(0.3), f32(-0.0), f32(-1.0)):                    # constant children: the constant itself, exactly
        t = np.full((8, 8, 8, 8), v, f32)
        w = np.full((8, 8, 8, 8), 5, f32)
        c = np.broadcast_to(np.array((10, 200, 33), np.uint8), (8, 8, 8, 8, 3)).copy() if color else None
        got, _ = halved_into_empty((m[0], t, w, c), color)
        assert np.all(u32(got[1]) == u32(np.array([v]))[0]) and np.all(got[2] == 5)
        assert not color or np.all(got[3] == np.array((10, 200, 33), np.uint8))


# ---- 3. a plane ----------------------------------------------------------------------------------------------------------------------------------------------
PLANE_BRICKS = (6, 2, 2)                                          # fine bricks from key (0, 0, 0) on


def plane_value(x):
    """the truncated SDF at position x (fine voxels): dyadic for x a multiple of 1 / 4"""
    return np.clip((np.asarray(x, f64) - 20.25) / 4.0, -1.0, 1.0)


def plane_map():
    bz, by, bx = np.meshgrid(np.arange(PLANE_BRICKS[2]), np.arange(PLANE_BRICKS[1]), np.arange(PLANE_BRICKS[0]), indexing="ij")
    keys = np.stack([bx, by, bz], -1).reshape(-1, 3).astype(np.int32)
    x = keys[:, 0, None] * 8 + np.arange(8)[None]                 # the fine world voxel per (brick, in-brick x)
    t = np.broadcast_to(plane_value(x + 0.5).astype(f32)[:, None, None, :], (len(keys), 8, 8, 8)).copy()
    assert np.array_equal(t.astype(f64), np.broadcast_to(plane_value(x + 0.5)[:, None, None, :], t.shape))       # the values are exact in fp32
    return np.ascontiguousarray(keys), t, np.ones_like(t), None


def plane_expectation(keys):
    """for the coarse bricks `keys`: the formula at the coarse centre 2 g + 1 (fine voxels), and which coarse voxels have both x-children strictly inside the band"""
    g = keys[:, 0, None].astype(np.int64) * 8 + np.arange(8)[None]
    inside = (np.abs(plane_value(2 * g + 0.5)) < 1) & (np.abs(plane_value(2 * g + 1.5)) < 1)
    shape = (len(keys), 8, 8, 8)
    return np.broadcast_to(plane_value(2 * g + 1.0)[:, None, None, :], shape), np.broadcast_to(inside[:, None, None, :], shape)


def test_plane_count_needs_no_device():
    keys = K.halved_brick_keys(plane_map()[0])
    assert len(keys) == 3 and np.count_nonzero(plane_expectation(keys)[1]) == 4 * 8 * 8         # coarse x = 8 .. 11


def test_a_plane_is_halved_exactly():
    m = plane_map()
    got, counts = halved_into_empty(m, False)
    assert counts == (3, 0, 0) and np.array_equal(got[0], K.halved_brick_keys(m[0]))
    want, inside = plane_expectation(got[0])
    assert np.count_nonzero(inside) == 256 and np.all(got[2] == 1)
    assert np.array_equal(got[1][inside].astype(f64), want[inside])


# ---- 4. a random sparse map ---------------------------------------------------------------------------------------------------------------------------------------
FAR = np.array((500000, -400000, 300000))
LONE = (20, 20, 20)                                               # a fine brick with no weight > 0, alone in its coarse brick
_SPARSE = {}


def sparse_map(color):
    """computed once and shared; nobody writes into the arrays"""
    if color not in _SPARSE:
        rng = np.random.default_rng(17)
        cells = rng.permutation(6 * 6 * 6)[:40]
        near = np.stack([cells % 6 - 3, (cells // 6) % 6 - 3, cells // 36 - 3], -1)              # about 40 bricks, keys straddling 0
        cluster = np.array([(x, y, z) for z in range(2) for y in range(2) for x in range(4)]) + FAR   # two coarse bricks with all eight children
        m = random_bricks(rng, np.concatenate([near, cluster, np.array([LONE])]), color)
        m[2][-1] = 0                                              # ... LONE: never observed
        quiet = 3                                                 # ... and a brick without a weight beside observed siblings or not, wherever it fell
        m[2][quiet] = 0
        counts = [0] * 9
        want = np_halve(m, counts)
        _SPARSE[color] = (m, want, counts)
    return _SPARSE[color]


@pytest.mark.parametrize("color", COLORS)
def test_a_random_sparse_map(color):
    m, want, counts = sparse_map(color)
    print("coarse voxels per number of observed children", counts, "coarse bricks", len(want[0]), "of", len(K.halved_brick_keys(m[0])))
    assert all(counts) and np.any(u32(m[1])[m[2] > 0] == 0x80000000)                            # every n from 0 to 8; an observed -0.0
    assert want[0][:, 0].min() < 0 < want[0][:, 0].max() and want[0][:, 0].max() > 200000
    lone = tuple(np.array(LONE) >> 1)
    assert lone in {tuple(k) for k in K.halved_brick_keys(m[0]).tolist()} and lone not in keyset(want)       # a candidate that takes no slot
    got, held = halved_into_empty(m, color)
    assert held == (len(want[0]), 0, 0)
    assert np.array_equal(got[0], want[0]) and same_store(got, want)


# ---- 5. the two fused sessions: halve A, then halve B into it ---------------------------------------------------------------------------------------------------------
_HALVED = {}


def halved_session(color, which):
    if (color, which) not in _HALVED:
        _HALVED[(color, which)] = np_halve(MM.session_map(64, color, which))
    return _HALVED[(color, which)]


@pytest.mark.parametrize("color", COLORS)
@pytest.mark.parametrize("first,second", [("A", "B"), ("B", "A")])
def test_two_sessions_halved_into_one_store(color, first, second):
    two_maps(64, color)
    a, b = MM.session_map(64, color, first), MM.session_map(64, color, second)
    ha, hb = halved_session(color, first), halved_session(color, second)
    want = np_merge(ha, hb)
    ia = {tuple(k): i for i, k in enumerate(ha[0].tolist())}
    both = sum(int(np.count_nonzero((ha[2][ia[tuple(k)]] > 0) & (hb[2][i] > 0))) for i, k in enumerate(hb[0].tolist()) if tuple(k) in ia)
    print(color, first, "<-", second, "coarse bricks", len(ha[0]), len(hb[0]), "merged", len(want[0]), "voxels with two weights", both)
    assert both >= 1000 and keyset(hb) - keyset(ha)
    ctx = MM.store_ctx(64, color)
    ctx.merge_brick_store_halved(a[0], a[1], a[2], a[3])
    assert same_store(store_sorted(ctx), ha)
    ctx.merge_brick_store_halved(b[0], b[1], b[2], b[3])
    assert same_store(store_sorted(ctx), want) and ctx.brick_store_count() == (len(want[0]), 0, 0)
    ctx.close()


def test_no_colour_given_on_a_colour_context():
    """a fresh slot's colour is 0, a held one's stays"""
    a, b = MM.session_map(64, True, "A"), MM.session_map(64, True, "B")
    ha, hb = halved_session(True, "A"), halved_session(True, "B")
    ctx = MM.store_ctx(64, True)
    ctx.merge_brick_store_halved(a[0], a[1], a[2], a[3])
    ctx.merge_brick_store_halved(b[0], b[1], b[2], None)
    assert same_store(store_sorted(ctx), np_merge(ha, hb, color_given=False))
    ctx.close()


def test_halved_onto_held_slots_with_a_pending_word():
    """the held path with deferred-weight words not 0: the halved bricks meet the TRUE weights, and the words left behind are 0.  The fine map is session
    B's, moved by whole fine bricks so that its coarse bricks start at the held bricks' least corner."""
    a, before = R.pending_store()
    b = MM.session_map(64, False, "B")
    off = 2 * before[0].min(axis=0) - b[0].min(axis=0)
    fine = sort_map((np.ascontiguousarray(b[0] + off.astype(np.int32)), b[1], b[2], None))
    hb = np_halve(fine)
    ia = {tuple(k): i for i, k in enumerate(before[0].tolist())}
    both = sum(int(np.count_nonzero((before[2][ia[tuple(k)]] > 0) & (hb[2][i] > 0))) for i, k in enumerate(hb[0].tolist()) if tuple(k) in ia)
    print("held", len(before[0]), "coarse incoming", len(hb[0]), "shared keys", len(keyset(before) & keyset(hb)), "voxels with two weights", both)
    assert keyset(before) & keyset(hb) and both > 0               # held keys are hit, and voxels blend
    a.merge_brick_store_halved(fine[0], fine[1], fine[2], None)
    want = np_merge(before, hb)
    first = store_sorted(a)
    assert same_store(first, want) and a.brick_store_count() == (len(want[0]), 0, 0) and not same_store(first, before)
    assert same_store(store_sorted(a), first)                     # a second read-out applies nothing twice
    a.close()


# ---- 6. order and run independence ----------------------------------------------------------------------------------------------------------------------------------
def test_order_and_context_play_no_part():
    m, want, _ = sparse_map(True)
    perm = np.random.default_rng(2).permutation(len(m[0]))
    shuffled = tuple(np.ascontiguousarray(x[perm]) for x in m)
    one, _ = halved_into_empty(m, True)
    two, _ = halved_into_empty(shuffled, True)
    assert same_store(one, two) and same_store(one, want)


# ---- 7. a full store ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_full_store_drops_and_keeps_held_keys_complete():
    m, want, _ = sparse_map(False)
    n = len(want[0])
    cap = n - 5
    got, counts = halved_into_empty(m, False, cap=cap)
    assert counts == (cap, 5, 0)
    at = {tuple(k): i for i, k in enumerate(want[0].tolist())}
    assert len(got[0]) == cap and keyset(got) <= keyset(want)
    for i, k in enumerate(got[0].tolist()):                       # every held key is complete: what the expectation gives it
        j = at[tuple(k)]
        assert np.array_equal(u32(got[1][i]), u32(want[1][j])) and np.array_equal(u32(got[2][i]), u32(want[2][j])), k


# ---- 8. bystanders ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bystanders_are_untouched():
    res, color = 64, False
    b = MM.session_map(res, color, "B")
    ctxs = [MM.session(res, color, "A") for _ in range(2)]       # the second one never sees the call
    trace = []
    for i, ctx in enumerate(ctxs):
        ctx.brick_store_capture()
        G.raycast(ctx, color)
        maps = lambda: [ctx.download_map(m, lv).copy() for m in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS) for lv in range(3)]
        planes, pose, origin, model, ntri = M.planes_bits(ctx, color), G.pose_of(ctx), ctx.volume_origin(), maps(), len(ctx.triangles())
        if i == 0:
            before = store_sorted(ctx)
            ctx.merge_brick_store_halved(b[0], b[1], b[2], None)
            assert not same_store(store_sorted(ctx), before)      # the store did change
            assert M.equal_bits(M.planes_bits(ctx, color), planes) and np.array_equal(u32(G.pose_of(ctx)), u32(pose)) and ctx.volume_origin() == origin
            assert all(G.same_bits(x, y) for x, y in zip(maps(), model)) and len(ctx.triangles()) == ntri
        follow = []
        for k in (6, 7):
            ok, p = G.run_frame(ctx, k, color)
            follow.append((ok, u32(p).copy(), M.planes_bits(ctx, color), [x.tobytes() for x in maps()]))
        trace.append(follow)
        ctx.close()
    for x, y in zip(*trace):                                      # the frames that follow
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and M.equal_bits(x[2], y[2]) and x[3] == y[3]


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    res = 64
    a, b = two_maps(res, False)
    ctx = MM.store_ctx(res, False, a)
    store, counts = store_sorted(ctx), ctx.brick_store_count()
    k2, t2, w2 = np.ascontiguousarray(b[0][:2]), np.ascontiguousarray(b[1][:2]), np.ascontiguousarray(b[2][:2])
    assert np.any(w2 > 0)
    twice = np.ascontiguousarray(np.stack([b[0][0], b[0][0]]))
    assert halved_raw(ctx, 2, twice, t2, w2, None) == ARG                                                  # a key twice in one call
    assert halved_raw(ctx, 2, None, t2, w2, None) == ARG and halved_raw(ctx, 2, k2, None, w2, None) == ARG and halved_raw(ctx, 2, k2, t2, None, None) == ARG
    for bad in ((1 << 20, 0, 0), (0, -(1 << 20) - 1, 0), (0, 0, 1 << 21)):
        far = np.ascontiguousarray(np.stack([b[0][0], np.array(bad, np.int32)]))
        assert halved_raw(ctx, 2, far, t2, w2, None) == ARG, bad                                          # a key out of range
    assert halved_raw(ctx, 2, k2, t2, w2, np.zeros((2, 512, 3), np.uint8)) == STATE                        # colour without a colour plane
    assert halved_raw(ctx, 0, None, None, None, None) == 0                                                 # nothing to merge: no array is looked at
    assert same_store(store_sorted(ctx), store) and ctx.brick_store_count() == counts
    ctx.close()
    bare = G.make_ctx(res)                                        # no store
    assert halved_raw(bare, 2, k2, t2, w2, None) == STATE and bare.brick_store_count() == (0, 0, 0)
    bare.close()
    slab = G.make_ctx(res, slab=(0, 32), halo=8)                  # a z-slab context
    G.fuse(slab, range(2))
    planes, pose = M.planes_bits(slab), G.pose_of(slab)
    assert halved_raw(slab, 2, k2, t2, w2, None) == ARG and slab.brick_store_count() == (0, 0, 0)
    assert M.equal_bits(M.planes_bits(slab), planes) and np.array_equal(u32(G.pose_of(slab)), u32(pose))
    slab.close()


# ---- 10. the host class -----------------------------------------------------------------------------------------------------------------------------------------------------
SIZE = 2.0


def header_fields(data):
    res, = struct.unpack_from("<I", data, 12)
    size, = struct.unpack_from("<f", data, 24)
    origin = struct.unpack_from("<3i", data, 32)
    pose = np.frombuffer(data, "<f4", 16, 48).reshape(4, 4).copy()
    return res, size, origin, pose


def coarse_origin(origin, levels):
    return tuple(8 * (int(o) // (8 << levels)) for o in origin)  # (Python's // is the floor division)


def coarse_pose(pose, size, res_file, origin, res_new, origin_new):
    """the translation moved by origin_file * s_file - origin_new * s_ctx metres, in float64, rounded to float32 once"""
    out = np.array(pose, f32)
    for k in range(3):
        out[k, 3] = f32((f64(out[k, 3]) + f64(origin[k]) * (f64(f32(size)) / f64(res_file))) - f64(origin_new[k]) * (f64(f32(size)) / f64(res_new)))
    return out


def write_expected(src_path, color, levels, path):
    """the file loadMapCoarser must be equivalent to loading: the records halved `levels` times by np_halve, the header's resolution, origin and pose as stated"""
    data = open(src_path, "rb").read()
    res, size, origin, pose = header_fields(data)
    m = MM.records(src_path, color)[0]
    for _ in range(levels):
        m = np_halve(m)
    new_res, new_origin = res >> levels, coarse_origin(origin, levels)
    new_pose = coarse_pose(pose, size, res, origin, new_res, new_origin)
    head = bytearray(data[:128])
    struct.pack_into("<I", head, 12, new_res)
    struct.pack_into("<3i", head, 32, *new_origin)
    head[48:112] = new_pose.astype("<f4").tobytes()
    struct.pack_into("<Q", head, 112, len(m[0]))
    with open(path, "wb") as f:
        f.write(bytes(head) + MM.record_bytes(m))
    return m, new_origin, new_pose


def relabelled(src_path, path, res=None, size=None, origin=None):
    """the same records under a header that names another resolution, size or origin"""
    head = bytearray(open(src_path, "rb").read())
    if res is not None:
        struct.pack_into("<I", head, 12, res)
    if size is not None:
        struct.pack_into("<f", head, 24, size)
    if origin is not None:
        struct.pack_into("<3i", head, 32, *origin)
    with open(path, "wb") as f:
        f.write(bytes(head))
    return path


def save_session(tmp_path, color, cam):
    path = str(tmp_path / "a64.hkfmap")
    a = MM.app_session(64, SIZE, cam, color, "A", CAP)
    try:
        assert a.save_map(path)
    finally:
        a.close()
    return path


def loaded_state(res, cam, color, path, coarser, frames=(6,)):
    """a fresh application of resolution `res` loads `path`; everything the comparison looks at, as bytes"""
    app = M.make_app(res, SIZE, cam, color)
    try:
        ok = app.load_map_coarser(path) if coarser else app.load_map(path)
        assert ok, path
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), res, SIZE)
        ctx.has_color = color
        out = dict(origin=app.volume_origin(), pose=u32(app.pose()[1]).copy(), device_pose=u32(G.pose_of(ctx)).copy(), frame_id=app.frame_id(),
                   planes=M.planes_bits(ctx, color), store=store_sorted(ctx), counts=app.brick_store_count()[:2],
                   model=[ctx.download_map(m, lv).tobytes() for m in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS) for lv in range(3)])
        ctx.clear_triangles()
        ctx.marching_cubes_map(300 * SIZE / res, has_color=color)
        out["triangles"] = ctx.triangles().tobytes()
        out["frames"] = []
        for k in frames:
            ok = M.app_frame(app, k, SIZE, cam, color)
            out["frames"].append((ok, u32(app.pose()[1]).copy(), M.planes_bits(ctx, color)))
    finally:
        app.close()
    return out


def assert_same_state(got, want):
    assert got["origin"] == want["origin"] and got["frame_id"] == want["frame_id"]
    assert np.array_equal(got["pose"], want["pose"]) and np.array_equal(got["device_pose"], want["device_pose"])
    assert same_store(got["store"], want["store"]) and got["counts"] == want["counts"]
    assert M.equal_bits(got["planes"], want["planes"])
    assert got["model"] == want["model"]
    assert got.get("triangles") == want.get("triangles")
    for x, y in zip(got["frames"], want["frames"]):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and M.equal_bits(x[2], y[2])


@pytest.mark.parametrize("color", COLORS)
def test_host_class_loads_a_finer_map(tmp_path, color):
    """resolution 64 -> 32 (the library takes 32)"""
    cam = G.RGB_CAM if color else G.CAM
    fine = save_session(tmp_path, color, cam)
    want_path = str(tmp_path / "want32.hkfmap")
    m, origin, pose = write_expected(fine, color, 1, want_path)
    assert origin == (16, 0, 0) and len(m[0]) > 20
    got = loaded_state(32, cam, color, fine, True)
    want = loaded_state(32, cam, color, want_path, False)
    assert got["origin"] == origin and np.array_equal(got["pose"], u32(pose)) and same_store(got["store"], m) and got["counts"] == (len(m[0]), 0)
    assert len(got["triangles"]) > 100 * 72 and np.count_nonzero(got["planes"][1]) > 1000
    print(color, "coarse bricks", len(m[0]), "triangles", len(got["triangles"]) // 72, "frame 6 tracked", got["frames"][0][0])
    assert_same_state(got, want)


# ---- 11. other ratios ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_class_other_ratios(tmp_path):
    color, cam = False, G.CAM
    fine = save_session(tmp_path, color, cam)
    # a ratio of 4: the same records under a header of resolution 128 and a negative origin, into an application of 32 -- two halvings
    f128 = relabelled(fine, str(tmp_path / "a128.hkfmap"), res=128, origin=(-40, 8, 40))
    want_path = str(tmp_path / "want32.hkfmap")
    m, origin, pose = write_expected(f128, color, 2, want_path)
    assert origin == (-16, 0, 8) and len(m[0]) >= 4 and np.count_nonzero(m[2] > 0) >= 100      # (64^3 voxels of surface at a quarter: not empty)
    got = loaded_state(32, cam, color, f128, True, frames=())
    want = loaded_state(32, cam, color, want_path, False, frames=())
    assert got["origin"] == origin and np.array_equal(got["pose"], u32(pose)) and same_store(got["store"], m)
    assert_same_state(got, want)
    # a ratio of 1 is load_map; a ratio of 3, of 16 or of 1 / 2, another size: refused with the application untouched
    refused = {"r3": relabelled(fine, str(tmp_path / "r3.hkfmap"), res=192), "r16": relabelled(fine, str(tmp_path / "r16.hkfmap"), res=1024),
               "half": relabelled(fine, str(tmp_path / "half.hkfmap"), res=32), "size": relabelled(fine, str(tmp_path / "size.hkfmap"), res=128, size=2.25),
               "missing": str(tmp_path / "missing.hkfmap")}
    app = M.make_app(64, SIZE, cam, color)
    try:
        app.set_brick_store(CAP)
        for k in range(3):
            assert M.app_frame(app, k, SIZE, cam, color), k
        assert app.shift_volume(32, 0, 0)
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), 64, SIZE)
        planes, store, counts, pose = M.planes_bits(ctx), store_sorted(ctx), app.brick_store_count(), app.pose()[1].copy()
        assert counts[0] > 0
        for name, p in refused.items():
            assert not app.load_map_coarser(p), name
            assert M.equal_bits(M.planes_bits(ctx), planes) and same_store(store_sorted(ctx), store) and app.brick_store_count() == counts, name
            assert app.volume_origin() == (32, 0, 0) and app.frame_id() == 2 and np.array_equal(u32(app.pose()[1]), u32(pose)), name
        assert app.load_map_coarser(fine) and app.volume_origin() == (32, 0, 0) and app.frame_id() == 5          # its own resolution: load_map
        assert same_store(store_sorted(ctx), MM.records(fine, color)[0])
    finally:
        app.close()


def test_slab_application_refuses(tmp_path):
    sl = H.SlabsApp(64, 2.0, G.CAM, [0, 32, 64])
    try:
        assert sl.load_map_coarser(str(tmp_path / "x.hkfmap")) is False
    finally:
        sl.close()


# ---- 12. the tool -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_tool_writes_the_halved_file(tmp_path):
    color, cam = False, G.CAM
    fine = save_session(tmp_path, color, cam)
    out_path, want_path = str(tmp_path / "lod.hkfmap"), str(tmp_path / "want32.hkfmap")
    spec = importlib.util.spec_from_file_location("map_lod", os.path.join(ROOT, "tools", "map_lod.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main([fine, out_path, "--levels", "1"]) == 0
    m, origin, pose = write_expected(fine, color, 1, want_path)
    info = H.map_file_info(out_path)                              # the reader accepts it: keys ascending, unique, in range, the length right
    assert (info["resolution"], info["has_color"], info["origin_vox"], info["n_bricks"]) == (32, color, origin, len(m[0]))
    assert np.array_equal(u32(info["pose"]), u32(pose))
    assert open(out_path, "rb").read() == open(want_path, "rb").read()
    got = loaded_state(32, cam, color, out_path, False, frames=())
    want = loaded_state(32, cam, color, fine, True, frames=())
    assert_same_state(got, want)
