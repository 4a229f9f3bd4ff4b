"""GPU: merging maps.  kf_merge_brick_store fuses a second map into the brick store voxel by voxel -- the reference's weighted running average
(tsdfVolume.h:65-70) applied map to map, exact in fp32 --, kf_refill_window re-reads the window from the store without capturing it first, and
HybKinectfu::mergeMap puts a map file behind both.  The yardstick is the numpy restatement of the rule below (np_rule, np_merge): float32 arrays, one
rounded operation per operation.  Shapes, stream and helpers are those of test_gpu_brickstore.py, test_gpu_shift.py and test_gpu_map_file.py: 64 voxels
at 2.0 m and 72 at 2.25 m, colour at 64, the 160 x 120 camera, Scene S, a store of 1024 bricks.  Everything is compared as integers, bit for bit.

The two sessions: A fuses frames 0-5 and shifts by (32, 0, 0); B fuses frames 0-8 and shifts by (0, 0, 16).  A session's map is its capture plus the
sorted read-out of its store.  Both sessions see the same box from nearly the same place, so they observe the same bricks; the store is therefore
reserved AFTER the shift: what the shift pushes out of the window is lost, A's map lacks the bricks with x < 4, B's those with z < 2, and the two maps
overlap in part only."""
import ctypes as C
import struct

import numpy as np
import pytest

import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_shift as G
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = B.u32
CAP = B.CAP
CASES = B.CASES
ARG, STATE = 1001, 1002
MAXW = G.P["volume_max_weight"]
SESSIONS = {"A": (range(6), (32, 0, 0)), "B": (range(9), (0, 0, 16))}


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------------------------
def np_rule(ta, wa, ca, tb, wb, cb, maxw):
    """a = held (true weights), b = incoming; arrays of voxels, colours (..., 3) uint8 or None (cb None: no colour given, the held colour stays)"""
    ta, wa, tb, wb = (np.asarray(x, f32) for x in (ta, wa, tb, wb))
    take = (wb > 0) & ~(wa > 0)                                   # only b observed: b verbatim
    blend = (wb > 0) & (wa > 0)
    s = np.where(blend, wa + wb, f32(1))                          # (a lane that does not blend divides by 1; its quotient is not used)
    t = np.where(blend, (ta * wa + tb * wb) / s, np.where(take, tb, ta))
    w = np.where(blend, np.minimum(wa + wb, f32(maxw)), np.where(take, wb, wa))
    assert t.dtype == f32 and w.dtype == f32 and s.dtype == f32
    c = None
    if ca is not None:
        c = ca.copy()
        if cb is not None:
            num = ca.astype(f32) * wa[..., None] + cb.astype(f32) * wb[..., None]
            assert num.dtype == f32
            cm = np.minimum(f32(255), num / s[..., None]).astype(np.uint8)      # (unsigned char) of a value in [0, 255]: truncation
            c = np.where(blend[..., None], cm, np.where(take[..., None], cb, ca))
    return t, w, c


def np_merge(a, b, maxw=MAXW, color_given=True):
    """map b merged into map a (each (keys, tsdf, weight, colour or None), keys unique): the sorted read-out the store must give"""
    color = a[3] is not None
    store = {tuple(k): (a[1][i], a[2][i], a[3][i] if color else None) for i, k in enumerate(a[0].tolist())}
    for i, k in enumerate(b[0].tolist()):
        tb, wb = b[1][i], b[2][i]
        cb = b[3][i] if (color and color_given and b[3] is not None) else None
        if not np.any(wb > 0):
            continue                                              # no weight > 0: nothing happens
        held = store.get(tuple(k))
        if held is None:
            store[tuple(k)] = (tb, wb, (cb if cb is not None else np.zeros((8, 8, 8, 3), np.uint8)) if color else None)
        else:
            store[tuple(k)] = np_rule(held[0], held[1], held[2], tb, wb, cb, maxw)
    keys = sorted(store, key=lambda k: (k[2], k[1], k[0]))
    return (np.array(keys, np.int32).reshape(-1, 3), np.stack([store[k][0] for k in keys]), np.stack([store[k][1] for k in keys]),
            np.stack([store[k][2] for k in keys]) if color else None)


# ---- the two sessions ------------------------------------------------------------------------------------------------------------------------------
def session(res, color, which, cap=CAP):
    frames, d = SESSIONS[which]
    ctx = G.make_ctx(res, color, 300000)
    G.fuse(ctx, frames, color)
    ctx.shift_volume(*d)                                          # no store yet: what leaves is gone
    ctx.brick_store_reserve(cap)
    return ctx


_MAPS = {}


def session_map(res, color, which):
    """computed once per shape and shared; nobody writes into the arrays"""
    if (res, color, which) not in _MAPS:
        ctx = session(res, color, which)
        ctx.brick_store_capture()
        m = B.store_sorted(ctx)
        assert ctx.brick_store_count() == (len(m[0]), 0, 0)
        ctx.close()
        for x in m:
            if x is not None:
                x.setflags(write=False)
        _MAPS[(res, color, which)] = m
    return _MAPS[(res, color, which)]


def keyset(m):
    return {tuple(k) for k in m[0].tolist()}


def two_maps(res, color):
    """both maps, after the assertion every test starts with: the four key classes are there, and enough voxels carry two weights"""
    a, b = session_map(res, color, "A"), session_map(res, color, "B")
    ka, kb = keyset(a), keyset(b)
    nb = res // 8
    in_window = {k for k in kb if 4 <= k[0] < 4 + nb and 0 <= k[1] < nb and 0 <= k[2] < nb}      # A's window stands at (32, 0, 0)
    ia = {tuple(k): i for i, k in enumerate(a[0].tolist())}
    both = sum(int(np.count_nonzero((a[2][ia[tuple(k)]] > 0) & (b[2][i] > 0))) for i, k in enumerate(b[0].tolist()) if tuple(k) in ia)
    print(res, color, "keys in both", len(ka & kb), "only A", len(ka - kb), "only B", len(kb - ka), "of B in A's window", len(in_window), "voxels with two weights", both)
    assert ka & kb and ka - kb and kb - ka and in_window and both >= 1000
    return a, b


def store_ctx(res, color, m=None, cap=CAP, **kw):
    """a fresh context with a store, holding map m"""
    ctx = G.make_ctx(res, color, **kw)
    ctx.brick_store_reserve(cap)
    if m is not None:
        ctx.write_brick_store(m[0], m[1], m[2], m[3])
    return ctx


def merge_raw(ctx, n, keys, t, w, c, off=None):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return ctx.lib.kf_merge_brick_store(ctx.h, n, p(keys), p(t), p(w), p(c), (C.c_int32 * 3)(*off) if off is not None else None)


def dense(m, origin, res, color):
    """the planes of a window at `origin` (voxels) filled from map m"""
    nb = res // 8
    t, w = np.zeros((res, res, res), f32), np.zeros((res, res, res), f32)
    c = np.zeros((res, res, res, 3), np.uint8) if color else None
    tb, wb, cb = B.bricks(t), B.bricks(w), B.bricks(c) if color else None
    hits = 0
    for i, k in enumerate(m[0].tolist()):
        x, y, z = (k[j] - origin[j] // 8 for j in range(3))
        if 0 <= x < nb and 0 <= y < nb and 0 <= z < nb:
            tb[z, y, x], wb[z, y, x] = m[1][i], m[2][i]
            if color:
                cb[z, y, x] = m[3][i]
            hits += 1
    return t, w, c, hits


# ---- 1. against numpy ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_merge_against_numpy(res, color):
    a, b = two_maps(res, color)
    m = store_ctx(res, color, a)
    n = len(b[0])
    order = np.random.default_rng(5).permutation(n)
    cut = (n // 2) | 1                                            # an odd index
    for part in (order[:cut], order[cut:]):
        m.merge_brick_store(b[0][part], b[1][part], b[2][part], b[3][part] if color else None)
    want = np_merge(a, b)
    assert M.same_store(B.store_sorted(m), want) and m.brick_store_count() == (len(want[0]), 0, 0)
    assert len(want[0]) == len(keyset(a) | keyset(b))
    m.close()


# ---- 2. synthetic bricks: every branch in one brick ---------------------------------------------------------------------------------------------------
def synthetic():
    """all normal numbers, no subnormal intermediate: tsdf k / 64, weights small integers, so every product and sum is a normal fp32"""
    rng = np.random.default_rng(11)
    tsdf = lambda: (rng.choice(np.concatenate([np.arange(-64, 0), np.arange(1, 65)]), 512).astype(f32) / f32(64)).reshape(8, 8, 8)
    ta, tb = tsdf(), tsdf()
    wa = rng.choice(np.array([0, 1, 2, 3, 7, 50, 100, 128], f32), 512).reshape(8, 8, 8)
    wb = rng.choice(np.array([0, 1, 2, 5, 30, 100, 128], f32), 512).reshape(8, 8, 8)
    ca, cb = rng.integers(0, 256, (8, 8, 8, 3), dtype=np.uint8), rng.integers(0, 256, (8, 8, 8, 3), dtype=np.uint8)
    # forced voxels: wa = 0 < wb with tb = -0.0; wb = 0 < wa; both with a clamped sum; channels 0 and 255 on both sides of a blend
    wa[0, 0, 0], wb[0, 0, 0], tb[0, 0, 0] = 0, 5, f32(-0.0)
    wa[0, 0, 1], wb[0, 0, 1] = 7, 0
    wa[0, 0, 2], wb[0, 0, 2] = 100, 100
    wa[0, 0, 3], wb[0, 0, 3], ca[0, 0, 3], cb[0, 0, 3] = 3, 5, (0, 255, 255), (0, 255, 0)
    wa[0, 0, 4], wb[0, 0, 4] = 0, 0
    return ta, wa, ca, tb, wb, cb


def test_synthetic_bricks_hit_every_branch():
    res, color = 64, True
    ta, wa, ca, tb, wb, cb = synthetic()
    assert np.any((wa == 0) & (wb > 0)) and np.any((wb == 0) & (wa > 0)) and np.any((wa > 0) & (wb > 0)) and np.any(wa + wb > MAXW)
    take = (wa == 0) & (wb > 0)
    assert np.any(take & (u32(tb) == 0x80000000))                 # a -0.0 to be copied verbatim
    blend = (wa > 0) & (wb > 0)
    assert np.any(ca[blend] == 0) and np.any(ca[blend] == 255) and np.any(cb[blend] == 0) and np.any(cb[blend] == 255)
    k_held, k_quiet, k_none, k_fresh = (1, 2, 3), (-4, 5, 6), (7, -8, 9), (-10, -11, 12)
    zeros = np.zeros((8, 8, 8), f32)
    held = (np.array([k_held, k_quiet], np.int32), np.stack([ta, ta]), np.stack([wa, wa]), np.stack([ca, ca]))
    o = np.lexsort((held[0][:, 0], held[0][:, 1], held[0][:, 2]))
    held = tuple(x[o] for x in held)
    incoming = (np.array([k_held, k_quiet, k_none, k_fresh], np.int32), np.stack([tb, tb, tb, tb]), np.stack([wb, zeros, zeros, wb]),
                np.stack([cb, cb, cb, cb]))
    ctx = store_ctx(res, color, held)
    assert ctx.brick_store_count() == (2, 0, 0)
    ctx.merge_brick_store(*incoming)
    want = np_merge(held, incoming)
    got = B.store_sorted(ctx)
    assert M.same_store(got, want) and ctx.brick_store_count() == (3, 0, 0)
    at = {tuple(k): i for i, k in enumerate(got[0].tolist())}
    assert k_none not in at                                       # an unheld key with no weight > 0: no slot
    q = at[k_quiet]                                               # a held key hit by an all-zero-weight entry: unchanged
    assert np.array_equal(u32(got[1][q]), u32(ta)) and np.array_equal(u32(got[2][q]), u32(wa)) and np.array_equal(got[3][q], ca)
    h = at[k_held]
    assert u32(got[1][h])[0, 0, 0] == 0x80000000 and got[2][h][0, 0, 0] == 5 and tuple(got[3][h][0, 0, 0]) == tuple(cb[0, 0, 0])
    assert u32(got[1][h])[0, 0, 1] == u32(ta)[0, 0, 1] and got[2][h][0, 0, 1] == 7 and tuple(got[3][h][0, 0, 1]) == tuple(ca[0, 0, 1])
    assert got[2][h][0, 0, 2] == MAXW and tuple(got[3][h][0, 0, 3]) == (0, 255, int(np.uint8(f32(255 * 3) / f32(8))))
    assert np.array_equal(u32(got[1][at[k_fresh]]), u32(tb)) and np.array_equal(got[3][at[k_fresh]], cb)   # a fresh key: verbatim
    # no colour given on the colour context: a held slot keeps its colour, a fresh one gets zeros
    k_fresh2 = (20, 21, -22)
    second = (np.array([k_held, k_fresh2], np.int32), np.stack([ta, tb]), np.stack([wb, wb]), None)
    ctx.merge_brick_store(second[0], second[1], second[2], None)
    want2 = np_merge(want, second, color_given=False)
    got2 = B.store_sorted(ctx)
    assert M.same_store(got2, want2) and ctx.brick_store_count() == (4, 0, 0)
    at2 = {tuple(k): i for i, k in enumerate(got2[0].tolist())}
    assert np.array_equal(got2[3][at2[k_held]], got[3][h]) and not np.any(got2[3][at2[k_fresh2]])
    assert not np.array_equal(u32(got2[1][at2[k_held]]), u32(got[1][h]))                                   # ... while tsdf and weight did merge
    ctx.close()


# ---- 3. into an empty store: a write ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_merge_into_an_empty_store_is_a_write(res, color):
    a, _ = two_maps(res, color)
    m, w = store_ctx(res, color), store_ctx(res, color, a)
    m.merge_brick_store(a[0], a[1], a[2], a[3])
    assert M.same_store(B.store_sorted(m), B.store_sorted(w)) and M.same_store(B.store_sorted(m), a)
    assert m.brick_store_count() == w.brick_store_count() == (len(a[0]), 0, 0)
    m.close(); w.close()


# ---- 4. commutative ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_merge_commutes(res, color):
    a, b = two_maps(res, color)
    ma, mb = store_ctx(res, color, a), store_ctx(res, color, b)
    ma.merge_brick_store(b[0], b[1], b[2], b[3])
    mb.merge_brick_store(a[0], a[1], a[2], a[3])
    assert M.same_store(B.store_sorted(ma), B.store_sorted(mb)) and ma.brick_store_count() == mb.brick_store_count()
    ma.close(); mb.close()


# ---- 5. offset ---------------------------------------------------------------------------------------------------------------------------------------
def test_offset_translates_the_keys():
    res, color = 64, False
    a, b = two_maps(res, color)
    for off in ((3, -2, 5), (1, 0, -1)):                          # the second one still collides with A's keys
        moved = np.ascontiguousarray(b[0] + np.array(off, np.int32))
        assert off == (3, -2, 5) or (keyset((moved,)) & keyset(a) and keyset((moved,)) - keyset(a))
        m1, m2 = store_ctx(res, color, a), store_ctx(res, color, a)
        m1.merge_brick_store(b[0], b[1], b[2], None, offset=off)
        assert merge_raw(m2, len(moved), moved, np.ascontiguousarray(b[1]), np.ascontiguousarray(b[2]), None, None) == 0      # NULL: zero
        o = np.lexsort((moved[:, 0], moved[:, 1], moved[:, 2]))
        want = np_merge(a, (moved[o], b[1][o], b[2][o], None))
        assert M.same_store(B.store_sorted(m1), want) and M.same_store(B.store_sorted(m2), want), off
        assert m1.brick_store_count() == m2.brick_store_count() == (len(want[0]), 0, 0), off
        if off != (1, 0, -1):
            m1.close(); m2.close()
    # one key pushed past 2^20 - 1: refused, store and counts untouched
    store, counts = B.store_sorted(m1), m1.brick_store_count()
    far = ((1 << 20) - int(b[0][:, 0].max()), 0, 0)
    kb, tb, wb = np.ascontiguousarray(b[0]), np.ascontiguousarray(b[1]), np.ascontiguousarray(b[2])
    assert merge_raw(m1, len(kb), kb, tb, wb, None, far) == ARG
    assert M.same_store(B.store_sorted(m1), store) and m1.brick_store_count() == counts
    assert merge_raw(m1, len(kb), kb, tb, wb, None, (far[0] - 1, 0, 0)) == 0           # ... and one brick less fits
    assert merge_raw(m2, len(kb), kb, tb, wb, None, (0, -(1 << 20) - 1 - int(b[0][:, 1].min()), 0)) == ARG
    assert merge_raw(m2, len(kb), kb, tb, wb, None, (0, 0, 2 ** 31 - 1)) == ARG        # no 32-bit wrap-around into the range
    assert M.same_store(B.store_sorted(m2), store) and m2.brick_store_count() == counts
    m1.close(); m2.close()


# ---- 6. held slots with a pending word ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,maxw", [(64, MAXW), (72, MAXW), (64, 4.0)])
def test_held_slots_with_a_pending_word(res, maxw):
    """A fuses with deferral forced on and its bricks leave by a shift, deferred-weight words with them.  The merge must start from the TRUE weights --
    what the read-out reported before -- and leave a word of 0: a second read-out applies nothing twice.  max_weight 4: quarters saturate within the six
    frames, the state in which word and stored weight differ most."""
    _, b = two_maps(res, False)
    a = K.Context(K.camera(*G.CAM), res, G.SIZES[res], maxw, levels=3)
    a.set_defer(1)
    a.brick_store_reserve(CAP)
    G.fuse(a, range(6))
    assert a.fusion_form()["defer"] == 1
    a.shift_volume(0, -24, 16)
    before = B.store_sorted(a)
    n = len(before[0])
    assert n >= 20 and a.brick_store_count() == (n, 0, 0) and keyset(before) & keyset(b)
    a.merge_brick_store(b[0], b[1], b[2])
    want = np_merge(before, b, maxw)
    first = B.store_sorted(a)
    assert M.same_store(first, want) and a.brick_store_count() == (len(want[0]), 0, 0)
    assert M.same_store(B.store_sorted(a), first)
    a.merge_brick_store(b[0][:1], b[1][:1], np.zeros_like(b[2][:1]))           # an entry without a weight goes by: still stable
    assert M.same_store(B.store_sorted(a), first)
    a.close()


# ---- 7. a full store -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_full_store_drops_new_keys_and_still_merges():
    res, color = 64, False
    a, b = two_maps(res, color)
    only_b = keyset(b) - keyset(a)
    assert len(only_b) > 3
    m = store_ctx(res, color, a, cap=len(a[0]) + 3)
    m.merge_brick_store(b[0], b[1], b[2])
    assert m.brick_store_count() == (len(a[0]) + 3, len(only_b) - 3, 0)
    got = B.store_sorted(m)
    want = np_merge(a, b)
    at = {tuple(k): i for i, k in enumerate(want[0].tolist())}
    new = keyset(got) - keyset(a)
    assert len(new) == 3 and new <= only_b and keyset(a) <= keyset(got)
    for i, k in enumerate(got[0].tolist()):                       # every held key -- colliding, only A's, or one of the three -- holds what the full merge gives it
        j = at[tuple(k)]
        assert np.array_equal(u32(got[1][i]), u32(want[1][j])) and np.array_equal(u32(got[2][i]), u32(want[2][j])), k
    m.close()


# ---- 8. refill ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_refill_shows_the_merged_store(res, color):
    am, b = two_maps(res, color)
    a = session(res, color, "A")
    a.brick_store_capture()
    assert M.same_store(B.store_sorted(a), am)
    a.merge_brick_store(b[0], b[1], b[2], b[3])
    want = np_merge(am, b)
    store, counts, pose, origin = B.store_sorted(a), a.brick_store_count(), G.pose_of(a), a.volume_origin()
    assert M.same_store(store, want) and origin == (32, 0, 0)
    t, w, c, hits = dense(want, origin, res, color)
    stale = M.planes_bits(a, color)
    assert not np.array_equal(stale[1], u32(w))                   # the window still shows A alone: the written keys are shadowed
    a.refill_window()
    B.assert_planes(a, color, t, w, c, "refill")                  # (with the observed-voxel count, re-based)
    assert np.array_equal(u32(G.pose_of(a)), u32(pose)) and a.volume_origin() == origin
    assert M.same_store(B.store_sorted(a), store)
    assert hits > 0 and a.brick_store_count() == (counts[0], counts[1], counts[2] + hits)
    a.close()


# ---- 9. derived state ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_derived_state_after_merge_and_refill(res, color):
    """A: capture, merge, refill.  C, fresh: the expected merged map written, the window placed at A's origin, A's pose.  A stale has-negative bit, skip
    table or deferred-weight word shows in the raycast, the extraction or the frames that follow."""
    am, b = two_maps(res, color)
    a = session(res, color, "A")
    c = G.make_ctx(res, color, 300000)
    c.brick_store_reserve(CAP)
    a.brick_store_capture()
    a.merge_brick_store(b[0], b[1], b[2], b[3])
    a.refill_window()
    want = np_merge(am, b)
    c.write_brick_store(want[0], want[1], want[2], want[3])
    c.place_window(*a.volume_origin())
    c.set_pose(G.pose_of(a))
    assert M.same_planes(a, c, color)
    G.raycast(a, color); G.raycast(c, color)
    G.assert_same_model(a, c, color)
    thr = 300 * a.size / res
    a.marching_cubes(thr, has_color=color)
    c.marching_cubes(thr, has_color=color)
    ta, tc = a.triangles(), c.triangles()
    assert len(ta) > 1000 and G.same_bits(ta, tc)
    for k in range(6, 10):
        oka, pa = G.run_frame(a, k, color)
        okc, pc = G.run_frame(c, k, color)
        assert oka == okc and np.array_equal(u32(pa), u32(pc)), (k, pa, pc)
    assert M.same_planes(a, c, color)
    a.close(); c.close()


# ---- 10. refill without capture forgets -------------------------------------------------------------------------------------------------------------------------------
def test_refill_without_capture_forgets():
    res = 64
    a = session(res, False, "A")
    a.shift_volume(16, 0, 0)
    a.shift_volume(-16, 0, 0)                                     # away and back: the bricks that left and returned are in the store, the others are not
    origin = a.volume_origin()
    store = B.store_sorted(a)
    held = keyset(store)
    _, w0, _ = G.planes(a)
    wb = B.bricks(w0)
    observed = {(x + origin[0] // 8, y + origin[1] // 8, z + origin[2] // 8) for z in range(8) for y in range(8) for x in range(8) if np.any(wb[z, y, x] > 0)}
    assert observed - held and observed & held                    # window-only bricks, and bricks the store holds too
    a.refill_window()
    t, w, _, hits = dense(store, origin, res, False)
    B.assert_planes(a, False, t, w, None, "refill without capture")
    wb = B.bricks(G.planes(a)[1])
    for k in observed - held:                                     # documented: a brick the store does not hold reads as never observed
        assert not np.any(wb[k[2] - origin[2] // 8, k[1] - origin[1] // 8, k[0] - origin[0] // 8]), k
    assert hits >= len(observed & held) and M.same_store(B.store_sorted(a), store)
    a.close()


# ---- 11. refusals touch nothing -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    res = 64
    _, b = two_maps(res, False)
    ctx = session(res, False, "A")
    ctx.brick_store_capture()                                     # a store with something in it
    store, planes, counts, origin, pose = B.store_sorted(ctx), M.planes_bits(ctx), ctx.brick_store_count(), ctx.volume_origin(), G.pose_of(ctx)
    k2, t2, w2 = np.ascontiguousarray(b[0][:2]), np.ascontiguousarray(b[1][:2]), np.ascontiguousarray(b[2][:2])
    twice = np.ascontiguousarray(np.stack([store[0][0], store[0][0]]))
    assert merge_raw(ctx, 2, twice, t2, w2, None) == ARG and merge_raw(ctx, 2, twice, t2, w2, None, (1, 1, 1)) == ARG      # a key twice in one call
    assert merge_raw(ctx, 2, None, t2, w2, None) == ARG and merge_raw(ctx, 2, k2, None, w2, None) == ARG and merge_raw(ctx, 2, k2, t2, None, None) == ARG
    assert merge_raw(ctx, 2, k2, t2, w2, np.zeros((2, 512, 3), np.uint8)) == STATE     # colour without a colour plane
    for bad in ((1 << 20, 0, 0), (0, -(1 << 20) - 1, 0), (0, 0, 1 << 21)):
        far = np.ascontiguousarray(np.stack([store[0][1], np.array(bad, np.int32)]))
        assert merge_raw(ctx, 2, far, t2, w2, None) == ARG, bad
    assert merge_raw(ctx, 0, None, None, None, None) == 0         # nothing to merge: no array is looked at
    assert M.same_store(B.store_sorted(ctx), store) and M.equal_bits(M.planes_bits(ctx), planes) and ctx.brick_store_count() == counts
    assert ctx.volume_origin() == origin and np.array_equal(u32(G.pose_of(ctx)), u32(pose))
    ctx.close()
    bare = G.make_ctx(res)                                        # no store
    G.fuse(bare, range(2))
    planes, pose = M.planes_bits(bare), G.pose_of(bare)
    assert merge_raw(bare, 2, k2, t2, w2, None) == STATE and bare.lib.kf_refill_window(bare.h) == STATE
    assert M.equal_bits(M.planes_bits(bare), planes) and bare.volume_origin() == (0, 0, 0) and bare.brick_store_count() == (0, 0, 0)
    assert np.array_equal(u32(G.pose_of(bare)), u32(pose))
    bare.close()
    slab = G.make_ctx(res, slab=(0, 32), halo=8)                  # a z-slab context: the store stays a whole-volume feature
    G.fuse(slab, range(2))
    planes, pose = M.planes_bits(slab), G.pose_of(slab)
    assert slab.lib.kf_refill_window(slab.h) == ARG and merge_raw(slab, 2, k2, t2, w2, None) == STATE
    assert M.equal_bits(M.planes_bits(slab), planes) and np.array_equal(u32(G.pose_of(slab)), u32(pose))
    slab.close()


# ---- 12. the host class ---------------------------------------------------------------------------------------------------------------------------------------------------
def records(path, color):
    data = open(path, "rb").read()
    rec = 12 + 4096 + (1536 if color else 0)
    n = (len(data) - 128) // rec
    assert len(data) == 128 + n * rec
    raw = np.frombuffer(data, np.uint8, offset=128).reshape(n, rec)
    keys = np.ascontiguousarray(raw[:, :12]).view("<i4").reshape(n, 3)
    t = np.ascontiguousarray(raw[:, 12:2060]).view("<f4").reshape(n, 8, 8, 8)
    w = np.ascontiguousarray(raw[:, 2060:4108]).view("<f4").reshape(n, 8, 8, 8)
    c = np.ascontiguousarray(raw[:, 4108:]).reshape(n, 8, 8, 8, 3) if color else None
    return (keys, t, w, c), data[128:]


def record_bytes(m):
    color = m[3] is not None
    parts = [m[0].astype("<i4").reshape(len(m[0]), -1).view(np.uint8), np.ascontiguousarray(m[1], "<f4").reshape(len(m[0]), -1).view(np.uint8),
             np.ascontiguousarray(m[2], "<f4").reshape(len(m[0]), -1).view(np.uint8)] + ([m[3].reshape(len(m[0]), -1)] if color else [])
    return np.concatenate(parts, axis=1).tobytes()


def app_session(res, size, cam, color, which, cap):
    frames, d = SESSIONS[which]
    app = M.make_app(res, size, cam, color)
    try:
        for k in frames:
            assert M.app_frame(app, k, size, cam, color), k
        assert app.shift_volume(*d)
        app.set_brick_store(cap)                                  # after the shift, as session() does
    except Exception:
        app.close()
        raise
    return app


@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_host_class_merges_two_sessions(tmp_path, res, color):
    size = G.SIZES[res]
    cam = G.RGB_CAM if color else G.CAM
    fa, fb, fab, fba = (str(tmp_path / (n + ".hkfmap")) for n in ("a", "b", "ab", "ba"))
    a = app_session(res, size, cam, color, "A", CAP)
    try:
        assert a.save_map(fa)
    finally:
        a.close()
    b = app_session(res, size, cam, color, "B", CAP)
    try:
        assert b.save_map(fb)
        ma, mb = records(fa, color)[0], records(fb, color)[0]
        assert keyset(ma) & keyset(mb) and keyset(ma) - keyset(mb) and keyset(mb) - keyset(ma)
        want = record_bytes(np_merge(ma, mb))
        assert want == record_bytes(np_merge(mb, ma))
        pose, frame_id, origin = b.pose()[1].copy(), b.frame_id(), b.volume_origin()
        assert b.merge_map(fa)
        assert np.array_equal(u32(b.pose()[1]), u32(pose)) and b.frame_id() == frame_id and b.volume_origin() == origin   # this session's, not the file's
        assert b.save_map(fba) and records(fba, color)[1] == want
        assert b.brick_store_count()[1] == 0
        assert M.app_frame(b, 9, size, cam, color)                # tracked against the merged model
    finally:
        b.close()
    small = len(ma[0]) + 5                                        # room for A's own capture, not for held + the file's bricks
    assert small < len(ma[0]) + len(mb[0])
    a = app_session(res, size, cam, color, "A", small)
    try:
        ca = K.Context.borrow(a.ctx_handle(), K.camera(*cam), res, size)
        assert a.merge_map(fb)
        held, dropped, _ = a.brick_store_count()
        assert dropped == 0 and held == len(keyset(ma) | keyset(mb))
        assert a.save_map(fab) and records(fab, color)[1] == want
        t, w, c, _ = dense(np_merge(ma, mb), (32, 0, 0), res, color)
        assert M.equal_bits(M.planes_bits(ca, color), (u32(t), u32(w), c))                                      # the window shows the merged map
        # foreign files: another resolution, size, max weight, colour flag -- refused with planes, store and pose untouched
        own = open(fb, "rb").read()
        foreign = {"res": own[:12] + struct.pack("<I", 72) + own[16:], "size": own[:24] + struct.pack("<f", 2.25) + own[28:],
                   "weight": own[:28] + struct.pack("<f", 64.0) + own[32:], "cut": own[:-1]}
        flipped = (mb[0], mb[1], mb[2], None if color else np.zeros((len(mb[0]), 8, 8, 8, 3), np.uint8))       # a well-formed file of the other kind
        foreign["colour"] = own[:20] + struct.pack("<I", 0 if color else 1) + own[24:128] + record_bytes(flipped)
        planes, store, counts, pose = M.planes_bits(ca, color), B.store_sorted(ca), a.brick_store_count(), a.pose()[1].copy()
        for name, data in foreign.items():
            p = str(tmp_path / (name + ".hkfmap"))
            with open(p, "wb") as f:
                f.write(data)
            assert not a.merge_map(p), name
            assert M.equal_bits(M.planes_bits(ca, color), planes) and M.same_store(B.store_sorted(ca), store) and a.brick_store_count() == counts, name
            assert np.array_equal(u32(a.pose()[1]), u32(pose)), name
        assert not a.merge_map(fb, offset=((1 << 20), 0, 0))      # a translated key out of range: refused the same way
        assert M.equal_bits(M.planes_bits(ca, color), planes) and M.same_store(B.store_sorted(ca), store) and a.brick_store_count() == counts
        assert M.app_frame(a, 6, size, cam, color)                # tracked against the merged model
    finally:
        a.close()
