"""GPU: erasing from the map.  kf_brick_store_erase_box clears a box of voxels in the brick store (or everything but the box), kf_brick_store_erase_weak
throws out bricks that were hardly observed; emptied bricks leave the store, the slots [0, held) stay dense, the table is rebuilt and freed slots are
handed out again.  HybKinectfu::eraseMapBox / eraseMapWeak put capture, erase and refill behind one call.  The yardstick is the numpy restatement below
(np_erase, np_weak) on the sorted read-out taken just before the call: voxel world coordinates from key * 8 + (x, y, z), cleared voxels zero, bricks without
a weight > 0 deleted.  Shapes, stream and helpers are those of test_gpu_brickstore.py, test_gpu_shift.py and test_gpu_map_merge.py: 64 voxels at 2.0 m
and 72 at 2.25 m, colour at 64, the 160 x 120 camera, 6 fused frames of Scene S, a store of 1024 bricks.  Everything is compared as integers, bit for bit."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_map_merge as MM
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
u32 = B.u32
CAP = B.CAP
CASES = B.CASES
ARG, STATE = 1001, 1002
LIM = 1 << 23                                                     # the key range in voxels: [-2^23, 2^23]
I32 = (-(1 << 31), (1 << 31) - 1)
INSIDE, OUTSIDE = K.ERASE_INSIDE, K.ERASE_OUTSIDE


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------------------------
def voxel_coords(keys):
    """world voxel coordinates (gx, gy, gz), each (n, 8, 8, 8) in (z, y, x) order"""
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    return tuple(k[:, j][:, None, None, None] * 8 + a[None] for j, a in enumerate((x, y, z)))


def np_erase(m, lo, hi, mode):
    """map m = (keys, tsdf, weight, colour or None), sorted -> (the erased map, bricks removed, observed voxels cleared, the count of each brick class and
    cut_bricks: which bricks of m are cut and kept)"""
    keys, t, w, c = m
    n = len(keys)
    lo, hi = np.clip(np.asarray(lo, np.int64), -LIM, LIM), np.clip(np.asarray(hi, np.int64), -LIM, LIM)
    g = voxel_coords(keys)
    inside = np.zeros((n, 8, 8, 8), bool)
    if not np.any(lo >= hi):
        inside = np.ones((n, 8, 8, 8), bool)
        for j in range(3):
            inside &= (g[j] >= lo[j]) & (g[j] < hi[j])
    clear = inside if mode == INSIDE else ~inside
    cleared = int(np.count_nonzero(clear & (w > 0)))
    t2, w2 = np.where(clear, f32(0), t), np.where(clear, f32(0), w)
    c2 = np.where(clear[..., None], np.uint8(0), c) if c is not None else None
    n_clear = clear.reshape(n, -1).sum(axis=1)
    left = (w2 > 0).reshape(n, -1).any(axis=1)
    cut = (n_clear > 0) & (n_clear < 512)
    classes = dict(whole=int(np.count_nonzero(n_clear == 512)), cut_kept=int(np.count_nonzero(cut & left)), cut_empty=int(np.count_nonzero(cut & ~left)),
                   untouched=int(np.count_nonzero(n_clear == 0)), cut_bricks=cut & left)
    assert np.all(left[n_clear == 0])                             # (a held brick has a weight > 0)
    return (keys[left], t2[left], w2[left], c2[left] if c is not None else None), int(n - np.count_nonzero(left)), cleared, classes


def np_weak(m, min_weight):
    keys, t, w, c = m
    keep = w.reshape(len(keys), -1).max(axis=1) >= f32(min_weight) if len(keys) else np.zeros(0, bool)
    return (keys[keep], t[keep], w[keep], c[keep] if c is not None else None), int(len(keys) - np.count_nonzero(keep))


def np_bounds(m):
    if len(m[0]) == 0:
        return (0, 0, 0), (0, 0, 0)
    return tuple(int(v) for v in m[0].min(axis=0)), tuple(int(v) for v in m[0].max(axis=0) + 1)


def assert_store_is(ctx, want, counts, what):
    got = B.store_sorted(ctx)
    assert np.array_equal(got[0], want[0]), what
    assert M.same_store(got, want), what
    assert ctx.brick_store_count() == counts, what
    assert ctx.brick_store_bounds() == np_bounds(want), what


def captured(res, color, shift=None, cap=CAP, max_triangles=0, defer=None):
    """a context whose store alone holds the map: 6 fused frames, captured; `shift`: the (empty) window is moved first, so the scene lies elsewhere in the world"""
    ctx = G.make_ctx(res, color, max_triangles)
    if defer is not None:
        ctx.set_defer(defer)
    ctx.brick_store_reserve(cap)
    if shift:
        ctx.shift_volume(*shift)
    G.fuse(ctx, range(6), color)
    ctx.brick_store_capture()
    return ctx


def search_box(m, mode, origin, whole=20, cut_kept=20, cut_empty=1, untouched=20):
    """an unaligned box (no face on a brick border) that removes >= `whole` bricks whole, cuts and keeps >= `cut_kept`, cuts >= `cut_empty` empty and
    leaves >= `untouched` untouched: the first of a fixed random sequence of boxes"""
    rng = np.random.default_rng(17)
    o = np.asarray(origin, np.int64)
    for _ in range(400):
        lo, hi = o + rng.integers(9, 31, 3), o + rng.integers(33, 56, 3)
        if np.any(lo % 8 == 0) or np.any(hi % 8 == 0):
            continue
        cl = np_erase(m, lo, hi, mode)[3]
        if cl["whole"] >= whole and cl["cut_kept"] >= cut_kept and cl["cut_empty"] >= cut_empty and cl["untouched"] >= untouched:
            return tuple(int(v) for v in lo), tuple(int(v) for v in hi)
    raise AssertionError("no box of the search meets the conditions")


def in_box(m, lo, hi):
    g = voxel_coords(m[0])
    inside = np.ones(m[1].shape, bool)
    for j in range(3):
        inside &= (g[j] >= lo[j]) & (g[j] < hi[j])
    return inside


def cut_quarters(m, lo, hi, quarter_is):
    """how many quarter bricks (the 128 voxels of z layers 2q, 2q + 1: in-brick index k >> 7) with the property quarter_is (n, 4) the box cuts: clears in part"""
    q_in = in_box(m, lo, hi).reshape(-1, 4, 128)
    return int(np.count_nonzero(q_in.any(axis=2) & ~q_in.all(axis=2) & quarter_is))


def search_quarter_box(m, quarter_is):
    """the box, of a fixed random sequence, that cuts the most quarters with the property"""
    rng = np.random.default_rng(29)
    best = (-1, None, None)
    for _ in range(200):
        lo = rng.integers(8, 44, 3)
        hi = lo + rng.integers(5, 40, 3)
        n = cut_quarters(m, lo, hi, quarter_is)
        if n > best[0]:
            best = (n, tuple(int(v) for v in lo), tuple(int(v) for v in hi))
    return best


# ---- 1. box against numpy --------------------------------------------------------------------------------------------------------------------------
BOXES = ["aligned", "unaligned", "negative", "everything", "beside", "empty"]


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("mode", [INSIDE, OUTSIDE])
@pytest.mark.parametrize("res,color", CASES)
def test_box_against_numpy(res, color, mode, box):
    shift = (-24, -24, -16) if box == "negative" else None
    ctx = captured(res, color, shift)
    m = B.store_sorted(ctx)
    n = len(m[0])
    assert n >= 100 and ctx.brick_store_count() == (n, 0, 0)
    origin = ctx.volume_origin()
    if box == "aligned":
        lo, hi = (24, 16, 8), (40, 48, 56)
    elif box in ("unaligned", "negative"):
        lo, hi = search_box(m, mode, origin)
    elif box == "everything":
        lo, hi = (I32[0],) * 3, (I32[1],) * 3
    elif box == "beside":
        lo, hi = (200, 200, 200), (I32[1], 300, 300)
    else:
        lo, hi = (10, 40, 10), (50, 40, 50)                       # lo == hi on y
    want, removed, cleared, cl = np_erase(m, lo, hi, mode)
    print(res, color, mode, box, lo, hi, "bricks", n, {k: v for k, v in cl.items() if k != "cut_bricks"}, "removed", removed, "cleared", cleared)
    # the case does what it is for
    if box == "aligned":
        assert cl["whole"] >= 20 and cl["untouched"] >= 20 and cl["cut_kept"] == 0 and cl["cut_empty"] == 0
    elif box in ("unaligned", "negative"):
        assert cl["whole"] >= 20 and cl["cut_kept"] >= 20 and cl["cut_empty"] >= 1 and cl["untouched"] >= 20
        assert all(v % 8 for v in lo + hi)
        if box == "negative":
            assert origin == shift and m[0].min() < 0 and min(lo) < 0
            assert (-1) >> 3 == -1 and (-9) >> 3 == -2            # the floor rule the keys follow
    elif (box == "everything") == (mode == INSIDE):
        assert cl["whole"] == n and removed == n and len(want[0]) == 0
    else:
        assert cl["untouched"] == n and removed == 0 and cleared == 0
    assert removed == cl["whole"] + cl["cut_empty"]
    got = ctx.brick_store_erase_box(lo, hi, mode)
    assert got == (removed, cleared), (got, removed, cleared)
    assert_store_is(ctx, want, (n - removed, 0, 0), (box, mode))
    ctx.close()


# ---- 2. the table really is rebuilt -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_the_table_is_rebuilt(res, color):
    """the store reserved at exactly the bricks the capture holds: the densest table the design allows, so probe chains are long"""
    probe = captured(res, color)
    n = probe.brick_store_count()[0]
    probe.close()
    ctx = captured(res, color, cap=n)
    m = B.store_sorted(ctx)
    assert ctx.brick_store_count() == (n, 0, 0) and len(m[0]) == n
    lo, hi = (I32[0],) * 3, (32, I32[1], I32[1])                 # a half space on a brick border: about half the bricks go, none is cut
    want, removed, cleared, cl = np_erase(m, lo, hi, INSIDE)
    print(res, color, "bricks", n, "removed", removed)
    assert n // 4 <= removed <= 3 * n // 4 and cl["cut_kept"] == 0 and cl["cut_empty"] == 0
    assert ctx.brick_store_erase_box(lo, hi, INSIDE) == (removed, cleared)
    assert_store_is(ctx, want, (n - removed, 0, 0), "erased")
    ctx.refill_window()                                           # every kept key is found, no removed key is
    t, w, c, hits = MM.dense(want, (0, 0, 0), res, color)
    assert hits == n - removed
    B.assert_planes(ctx, color, t, w, c, "refilled")
    gone = ~np.isin(B_words(m[0]), B_words(want[0]))
    assert np.count_nonzero(gone) == removed
    ctx.write_brick_store(m[0][gone], m[1][gone], m[2][gone], m[3][gone] if color else None)     # exactly those bricks come back, into the freed slots
    assert_store_is(ctx, m, (n, 0, hits), "written back")            # (`restored` counts the bricks the refill has read back; the erase left it alone)
    ctx.close()


def B_words(keys):
    k = np.asarray(keys, np.int64).reshape(-1, 3) + (1 << 20)
    return (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]


# ---- 3. slots come back ---------------------------------------------------------------------------------------------------------------------------------
def fresh_bricks(n, first, color):
    keys = np.array([[1000 + first + i, -7, 3] for i in range(n)], np.int32)
    t = np.full((n, 8, 8, 8), f32(0.25))
    w = np.full((n, 8, 8, 8), f32(3))
    return keys, t, w, (np.full((n, 8, 8, 8, 3), 9, np.uint8) if color else None)


@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_slots_come_back(res, color):
    probe = captured(res, color)
    n = probe.brick_store_count()[0]
    probe.close()
    ctx = captured(res, color, cap=n)
    assert ctx.brick_store_count() == (n, 0, 0)
    ctx.write_brick_store(*fresh_bricks(1, 0, color))             # the store is full: dropped
    assert ctx.brick_store_count() == (n, 1, 0)
    m = B.store_sorted(ctx)
    lo, hi = (11, 13, I32[0]), (51, 53, 35)
    want, removed, cleared, _ = np_erase(m, lo, hi, INSIDE)
    assert removed >= 20
    assert ctx.brick_store_erase_box(lo, hi, INSIDE) == (removed, cleared)
    assert ctx.brick_store_count() == (n - removed, 1, 0)
    fresh = fresh_bricks(removed, 1, color)
    ctx.write_brick_store(*fresh)                                 # as many fresh keys as bricks were removed: every one takes a freed slot
    assert ctx.brick_store_count() == (n, 1, 0)
    ctx.write_brick_store(*fresh_bricks(1, removed + 1, color))   # one more: dropped again
    assert ctx.brick_store_count() == (n, 2, 0)
    both = MM.np_merge(want, fresh)                               # (disjoint keys: a plain union, sorted)
    assert M.same_store(B.store_sorted(ctx), both)
    ctx.close()


# ---- 4. derived state --------------------------------------------------------------------------------------------------------------------------------------
def cut_box(res):
    """through the back wall and the free space in front of it, no face on a brick border"""
    return (19, 21, 27), (43, 45, res - 3)


def negatives(m):
    return int(np.count_nonzero((m[1] < 0) & (m[2] > 0)))


@pytest.mark.parametrize("res,color", CASES)
def test_derived_state(res, color):
    a = captured(res, color, max_triangles=300000)
    b = G.make_ctx(res, color, 300000)
    m = B.store_sorted(a)
    lo, hi = cut_box(res)
    want, removed, cleared, cl = np_erase(m, lo, hi, INSIDE)
    print(res, color, "voxels behind the surface", negatives(m), "->", negatives(want))
    assert cl["cut_kept"] >= 20 and negatives(m) - negatives(want) >= 100 and negatives(want) >= 100     # the box cuts the surface: part goes, part stays
    assert a.brick_store_erase_box(lo, hi, INSIDE) == (removed, cleared)
    a.refill_window()
    t, w, c, _ = MM.dense(want, (0, 0, 0), res, color)
    B.assert_planes(a, color, t, w, c, "refilled")
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
    a.close(); b.close()


# ---- 5. going on, with deferral -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 72])
def test_going_on_with_deferral(res):
    """A defers whole-quarter free-space weights, B never does.  The box cuts free-space bricks in front of the wall: a deferred-weight word left at 1 on a
    cut quarter would let A's next deferred step count on voxels that are no longer observed, and frames 6-9 would differ."""
    a, b = captured(res, False, defer=1), G.make_ctx(res)
    b.set_defer(0)
    assert a.fusion_form()["defer"] == 1
    m = B.store_sorted(a)
    # the quarters deferral works on: all 128 voxels observed, all at tsdf 1 -- free space in front of the wall.  The box cuts as many as it can find
    free = ((m[2] > 0) & (m[1] == 1)).reshape(-1, 4, 128).all(axis=2)
    n_free, lo, hi = search_quarter_box(m, free)
    want, removed, cleared, cl = np_erase(m, lo, hi, INSIDE)
    print(res, lo, hi, "free-space quarters", int(np.count_nonzero(free)), "of them cut", n_free, "bricks cut and kept", cl["cut_kept"], "voxels cleared", cleared)
    assert n_free >= 4 and cl["cut_kept"] >= 4 and cleared >= 500
    assert a.brick_store_erase_box(lo, hi, INSIDE) == (removed, cleared)
    a.refill_window()
    t, w, _, _ = MM.dense(want, (0, 0, 0), res, False)
    B.assert_planes(a, False, t, w, None, "refilled")
    b.upload_volume(t, w)
    b.set_pose(G.pose_of(a))
    G.raycast(a); G.raycast(b)
    for k in range(6, 10):
        oka, pa = G.run_frame(a, k)
        okb, pb = G.run_frame(b, k)
        assert oka and okb, k
        assert np.array_equal(u32(pa), u32(pb)), (k, pa, pb)
        assert a.fusion_form()["defer"] == 1 and b.fusion_form()["defer"] == 0
    assert M.same_planes(a, b)
    a.close(); b.close()


# ---- 6. saturated quarters -----------------------------------------------------------------------------------------------------------------------------------
def test_saturated_quarters():
    """max_weight 2 and deferral: after 6 frames the free-space quarters are saturated, and the flush before the capture leaves them with KF_PEND_SAT -- under
    which a stored weight of 0 would read as max_weight.  The test cannot see the word; it sees that every cleared voxel reads 0."""
    res, maxw = 64, 2.0
    ctx = K.Context(K.camera(*G.CAM), res, G.SIZES[res], maxw, levels=3)
    ctx.set_defer(1)
    ctx.brick_store_reserve(CAP)
    G.fuse(ctx, range(6))
    assert ctx.fusion_form()["defer"] == 1
    ctx.brick_store_capture()
    m = B.store_sorted(ctx)
    sat = np.all(m[2].reshape(-1, 4, 128) == f32(maxw), axis=2)   # the quarters that carry KF_PEND_SAT after the flush: every weight at max_weight
    sat_cut, lo, hi = search_quarter_box(m, sat)
    want, removed, cleared, cl = np_erase(m, lo, hi, INSIDE)
    print(lo, hi, "saturated quarters", int(np.count_nonzero(sat)), "of them cut by the box", sat_cut)
    assert sat_cut >= 10
    assert ctx.brick_store_erase_box(lo, hi, INSIDE) == (removed, cleared)
    assert_store_is(ctx, want, (len(m[0]) - removed, 0, 0), "saturated")
    ctx.refill_window()
    t, w, _, _ = MM.dense(want, (0, 0, 0), res, False)
    B.assert_planes(ctx, False, t, w, None, "saturated, refilled")
    wz = w[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    assert not np.any(wz) and np.count_nonzero(w) == np.count_nonzero(m[2] > 0) - cleared
    ctx.close()


# ---- 7. weak against numpy -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_weak_against_numpy(res, color):
    """the window moves on after 6 frames and sees 3 more: the bricks it has left stay at a weight of 6 at most, those it still holds go on to 9"""
    ctx = captured(res, color)
    ctx.shift_volume(32, 0, 0)
    G.raycast(ctx, color)
    for k in range(6, 9):
        ok, _ = G.run_frame(ctx, k, color)
        assert ok, k
    ctx.brick_store_capture()
    m = B.store_sorted(ctx)
    n = len(m[0])
    counts = ctx.brick_store_count()
    assert counts[:2] == (n, 0)
    top = m[2].reshape(n, -1).max(axis=1)
    split = [wt for wt in (2, 3, 4, 5, 6, 7, 8, 9) if np.count_nonzero(top < wt) >= 10 and np.count_nonzero(top >= wt) >= 50]
    print(res, color, "greatest weights", dict(zip(*[v.tolist() for v in np.unique(top, return_counts=True)])), "thresholds that split", split)
    assert split
    assert ctx.brick_store_erase_weak(0.0) == 0 and ctx.brick_store_erase_weak(-1.0) == 0
    assert_store_is(ctx, m, (n, 0, counts[2]), "min_weight <= 0")
    assert ctx.lib.kf_brick_store_erase_weak(ctx.h, float("nan"), None) == ARG
    want, removed = np_weak(m, split[0])
    assert removed >= 10 and len(want[0]) >= 50
    assert ctx.brick_store_erase_weak(split[0]) == removed
    assert_store_is(ctx, want, (n - removed, 0, counts[2]), "weak")        # the kept bricks bit for bit
    assert ctx.brick_store_erase_weak(split[0]) == 0               # nothing weak is left
    assert_store_is(ctx, want, (n - removed, 0, counts[2]), "weak, again")
    assert ctx.brick_store_erase_weak(1e9) == n - removed
    assert ctx.brick_store_count() == (0, 0, counts[2]) and len(ctx.brick_store()[0]) == 0 and ctx.brick_store_bounds() == ((0, 0, 0), (0, 0, 0))
    ctx.write_brick_store(m[0], m[1], m[2], m[3])                  # an emptied store takes a map again
    assert_store_is(ctx, m, (n, 0, counts[2]), "refilled store")
    ctx.close()


# ---- 8. bystander and refusals ------------------------------------------------------------------------------------------------------------------------------------
def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_bystander_and_refusals():
    res = 64
    a, b = captured(res, False), captured(res, False)
    assert a.brick_store_erase_box((200, 200, 200), (300, 300, 300), INSIDE) == (0, 0)
    assert a.brick_store_erase_box(I32[:1] * 3, I32[1:] * 3, OUTSIDE) == (0, 0)
    assert M.same_store(B.store_sorted(a), B.store_sorted(b)) and a.brick_store_count() == b.brick_store_count()
    assert M.same_planes(a, b) and np.array_equal(u32(G.pose_of(a)), u32(G.pose_of(b)))
    for k in range(6, 8):
        oka, pa = G.run_frame(a, k)
        okb, pb = G.run_frame(b, k)
        assert oka and okb and np.array_equal(u32(pa), u32(pb)), k
        assert M.same_planes(a, b), k
    b.close()
    lib, counts, store = a.lib, a.brick_store_count(), B.store_sorted(a)
    removed, cleared = C.c_uint32(5), C.c_uint64(5)
    assert lib.kf_brick_store_erase_box(None, i3(0, 0, 0), i3(64, 64, 64), 0, None, None) == ARG
    assert lib.kf_brick_store_erase_weak(None, 1.0, None) == ARG
    for mode in (2, -1):
        assert lib.kf_brick_store_erase_box(a.h, i3(0, 0, 0), i3(64, 64, 64), mode, C.byref(removed), C.byref(cleared)) == ARG
    assert lib.kf_brick_store_erase_box(a.h, None, i3(64, 64, 64), 0, None, None) == ARG
    assert lib.kf_brick_store_erase_box(a.h, i3(0, 0, 0), None, 0, None, None) == ARG
    assert a.brick_store_count() == counts and M.same_store(B.store_sorted(a), store)
    assert lib.kf_brick_store_erase_box(a.h, i3(0, 0, 0), i3(64, 64, 64), 1, None, None) == 0        # the out-pointers may be NULL
    assert a.brick_store_count() == counts
    a.close()
    bare = G.make_ctx(res)                                        # no store
    G.fuse(bare, range(2))
    planes = M.planes_bits(bare)
    assert bare.lib.kf_brick_store_erase_box(bare.h, i3(0, 0, 0), i3(64, 64, 64), 0, None, None) == STATE
    assert bare.lib.kf_brick_store_erase_weak(bare.h, 2.0, None) == STATE
    assert bare.brick_store_count() == (0, 0, 0) and M.equal_bits(M.planes_bits(bare), planes)
    bare.close()
    slab = G.make_ctx(res, slab=(0, 32), halo=8)
    assert slab.lib.kf_brick_store_erase_box(slab.h, i3(0, 0, 0), i3(64, 64, 64), 0, None, None) == ARG
    assert slab.lib.kf_brick_store_erase_weak(slab.h, 2.0, None) == ARG
    assert slab.brick_store_count() == (0, 0, 0)
    slab.close()


# ---- 9. the map mesh ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_the_map_mesh(res, color):
    a = captured(res, color, max_triangles=300000)
    m = B.store_sorted(a)
    lo, hi = cut_box(res)
    want, removed, cleared, _ = np_erase(m, lo, hi, INSIDE)
    assert negatives(m) - negatives(want) >= 100 and negatives(want) >= 100
    assert a.brick_store_erase_box(lo, hi, INSIDE) == (removed, cleared)
    a.refill_window()                                             # the window shadows the store: it must show the erased map too
    b = G.make_ctx(res, color, 300000)                            # a fresh context: its empty window stands where the map is not
    b.brick_store_reserve(CAP)
    b.shift_volume(32 * res, 0, 0)
    b.write_brick_store(want[0], want[1], want[2], want[3])
    thr = 300 * a.size / res
    ta, tb = [], []
    for ctx, out in ((a, ta), (b, tb)):
        ctx.clear_triangles()
        ctx.marching_cubes_map(thr, has_color=color)
        out.append(ctx.triangles())
    print(res, color, "map triangles", len(ta[0]))
    assert len(ta[0]) > 0 and G.same_bits(ta[0], tb[0])
    a.close(); b.close()


# ---- 10. the host class -----------------------------------------------------------------------------------------------------------------------------------------------
def centre_rule(lo_m, hi_m, cell):
    """the test's own voxel box: voxel g is in iff lo <= (g + 1/2) * cell < hi, evaluated voxel by voxel in float64"""
    g = np.arange(-512, 512)
    centre = (g + 0.5) * float(cell)
    lo, hi = [], []
    for k in range(3):
        inside = g[(centre >= float(f32(lo_m[k]))) & (centre < float(f32(hi_m[k])))]
        assert len(inside)
        lo.append(int(inside[0])); hi.append(int(inside[-1]) + 1)
    return tuple(lo), tuple(hi)


@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_host_class_erases_in_metres(tmp_path, res, color):
    size = G.SIZES[res]
    cam = G.RGB_CAM if color else G.CAM
    cell = f32(size) / f32(res)
    f0, f1, f2 = (str(tmp_path / (n + ".hkfmap")) for n in ("before", "box", "weak"))
    app = M.make_app(res, size, cam, color)
    try:
        app.set_brick_store(CAP)
        for k in range(6):
            assert M.app_frame(app, k, size, cam, color), k
            if k == 2:
                assert app.shift_volume(32, 0, 0)
        assert app.save_map(f0)
        m0 = MM.records(f0, color)[0]
        want_lo, want_hi = search_box(m0, INSIDE, (0, 0, 0), whole=10, cut_empty=0)
        # WORLD metres, the first cube's coordinates, whatever the window's origin: a quarter cell above a voxel's lower border
        lo_m, hi_m = tuple(float((f32(v) + f32(0.25)) * cell) for v in want_lo), tuple(float((f32(v) + f32(0.25)) * cell) for v in want_hi)
        lo, hi = centre_rule(lo_m, hi_m, cell)
        assert (lo, hi) == (want_lo, want_hi) and all(v % 8 for v in lo + hi)
        want, removed, cleared, cl = np_erase(m0, lo, hi, INSIDE)
        print(res, color, lo_m, hi_m, lo, hi, {k: v for k, v in cl.items() if k != "cut_bricks"})
        assert cl["whole"] >= 10 and cl["cut_kept"] >= 20 and cl["untouched"] >= 20
        pose, frame_id, origin = app.pose()[1].copy(), app.frame_id(), app.volume_origin()
        assert app.erase_map_box(lo_m, hi_m) and app.erase_counts == (removed, cleared)
        assert np.array_equal(u32(app.pose()[1]), u32(pose)) and app.frame_id() == frame_id and app.volume_origin() == origin == (32, 0, 0)
        assert app.brick_store_count()[:2] == (len(want[0]), 0)
        assert app.save_map(f1) and MM.records(f1, color)[1] == MM.record_bytes(want)
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), res, size)
        t, w, c, _ = MM.dense(want, origin, res, color)
        assert M.equal_bits(M.planes_bits(ctx, color), (u32(t), u32(w), c))                               # the window shows the erased map
        assert M.app_frame(app, 6, size, cam, color)              # tracked against the erased model
        assert app.save_map(f2)
        m1 = MM.records(f2, color)[0]
        top = m1[2].reshape(len(m1[0]), -1).max(axis=1)
        split = [wt for wt in (2, 3, 4, 5, 6, 7) if np.count_nonzero(top < wt) >= 5 and np.count_nonzero(top >= wt) >= 50]
        assert split
        want_w, removed_w = np_weak(m1, split[0])
        assert app.erase_map_weak(split[0]) and app.erase_counts == (removed_w, 0)
        assert app.save_map(f2) and MM.records(f2, color)[1] == MM.record_bytes(want_w)
        assert M.app_frame(app, 7, size, cam, color)
        counts = app.brick_store_count()
        assert not app.erase_map_box((float("nan"), 0, 0), (1, 1, 1)) and not app.erase_map_weak(float("nan"))
        assert app.brick_store_count() == counts
        # keep_inside crops the map to the box
        assert app.save_map(f0)
        m2 = MM.records(f0, color)[0]
        want_c, removed_c, cleared_c, _ = np_erase(m2, lo, hi, OUTSIDE)
        assert app.erase_map_box(lo_m, hi_m, keep_inside=True) and app.erase_counts == (removed_c, cleared_c)
        assert app.save_map(f1) and MM.records(f1, color)[1] == MM.record_bytes(want_c)
        # tools/map_crop.py does the same to the file saved before the crop: the same records, the header but for the brick count
        spec = importlib.util.spec_from_file_location("map_crop", os.path.join(ROOT, "tools", "map_crop.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        assert tool.main([f0, f2, "--box"] + [repr(v) for v in lo_m + hi_m] + ["--outside"]) == 0
        assert MM.records(f2, color)[1] == MM.record_bytes(want_c)
        h0, h2 = open(f0, "rb").read(128), open(f2, "rb").read(128)
        assert h0[:112] == h2[:112] and h0[120:] == h2[120:] and H.map_file_info(f2)["n_bricks"] == len(want_c[0])
    finally:
        app.close()


def test_slab_application_refuses():
    sl = H.SlabsApp(64, 2.0, G.CAM, [0, 32, 64])
    try:
        assert sl.erase_map_box((0, 0, 0), (1, 1, 1)) is False and sl.erase_map_weak(2.0) is False
    finally:
        sl.close()
