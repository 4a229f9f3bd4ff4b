"""GPU: kf_marching_cubes_region -- marching cubes limited to a box of cells, appended to the triangle buffer (or the world soup), its cost
following the box.  The yardstick is the EXISTING whole-volume kf_marching_cubes on a masked volume (stream_common.masked_soup): a cell's
triangles depend on its 27 voxels alone, so the whole-volume extraction of a volume that is zero outside voxels [lo - 1, hi + 1) is, byte for
byte and in order, what the region extraction of the original volume must append.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import stream_common as T
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32 = np.float32
STRESS_THR = 1.0e9                                                # no threshold: every sign change counts
STRESS_MAX = 900000


def volume(kind, res, color):
    """(tsdf, weight, colour or None, threshold, max_triangles)"""
    if kind == "scene":
        t, w, c, _ = T.fused(res, color)
        return t, w, c, T.thr_of(res), T.MAX_TRI
    t, w = T.stress_volume(res, res)
    return t, w, (T.stress_color(res, res) if color else None), STRESS_THR, STRESS_MAX


def boxes(kind, R):
    """interior and unaligned; one cell thick on each axis; touching the three low / the three high faces (with bounds beyond the volume: clamped);
    the whole volume.  The scene's boxes are placed on its surfaces: the central sphere (radius 0.15 R) and the back wall at 0.75 R."""
    h = R // 2
    inner = ((3, 9, 17), (30, 41, 22)) if kind == "stress" else ((h - 13, 9, h - 15), (h + 14, h + 9, h - 2))
    return [inner,
            ((h + 1, 0, 0), (h + 2, R, R)), ((0, h + 1, 0), (R, h + 2, R)), ((0, 0, h - 6), (R, R, h - 5)),
            ((-5, -5, -5), (h + 3, h + 3, h + 3)), ((h - 5, h - 5, h - 5), (R + 9, R + 9, R + 9)),
            ((0, 0, 0), (R, R, R))]


CASES = [("scene", 64, False), ("scene", 72, False), ("scene", 64, True), ("scene", 72, True), ("stress", 40, False), ("stress", 64, False), ("stress", 40, True)]


# ---- 1. region == masked whole volume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,res,color", CASES)
def test_region_equals_masked_whole_volume(kind, res, color):
    t, w, c, thr, cap = volume(kind, res, color)
    ctx = T.ctx_with(res, t, w, c, max_triangles=cap)
    for lo, hi in boxes(kind, res):
        ctx.clear_triangles()
        ctx.marching_cubes_region(thr, lo, hi, has_color=color)
        got = ctx.triangles()
        want = T.masked_soup(res, t, w, c, lo, hi, thr, cap)
        print("%s %d color=%d box %s %s: %d triangles" % (kind, res, color, lo, hi, len(got)))
        assert len(want) > 0 and len(got) < cap, (lo, hi)         # an empty answer cannot pass
        assert T.same_bits(got, want), (lo, hi, len(got), len(want))
    ctx.close()


# ---- 2. partition --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,res", [("scene", 72), ("stress", 40)])
def test_partition(kind, res):
    t, w, c, thr, cap = volume(kind, res, False)
    ctx = T.ctx_with(res, t, w, max_triangles=cap)
    ctx.marching_cubes(thr)
    whole = ctx.triangles()
    assert 0 < len(whole) < cap
    R = res
    for axis, cut in ((0, 27), (1, R // 2 + 3), (2, R // 2 - 5)):
        parts = []
        for lo_k, hi_k in ((0, cut), (cut, R)):
            lo, hi = [0, 0, 0], [R, R, R]
            lo[axis], hi[axis] = lo_k, hi_k
            ctx.clear_triangles()
            ctx.marching_cubes_region(thr, lo, hi)
            parts.append(ctx.triangles())
        assert len(parts[0]) > 0 and len(parts[1]) > 0, axis
        assert len(parts[0]) + len(parts[1]) == len(whole), axis
        assert T.is_subsequence(parts[0], whole) and T.is_subsequence(parts[1], whole), axis
        assert np.array_equal(T.sorted_words(np.concatenate(parts)), T.sorted_words(whole)), axis
    ctx.close()


# ---- 3. append and clamp -------------------------------------------------------------------------------------------------------------------
def test_append_and_clamp():
    res = 64
    t, w, c, thr, cap = volume("scene", res, False)
    h = res // 2
    b1, b2 = ((0, 0, 0), (h + 3, res, res)), ((h - 5, 3, 0), (res, res - 2, res))      # overlapping boxes: the second call appends, it does not merge
    ctx = T.ctx_with(res, t, w, max_triangles=cap)
    ctx.marching_cubes_region(thr, *b1)
    first = ctx.triangles()
    ctx.marching_cubes_region(thr, *b2)
    both = ctx.triangles()
    ctx.clear_triangles()
    ctx.marching_cubes_region(thr, *b2)
    second = ctx.triangles()
    ctx.close()
    assert len(first) > 100 and len(second) > 100
    assert T.same_bits(both, np.concatenate([first, second]))
    small = len(first) + len(second) // 2                          # below the total: the second call's tail does not fit
    ctx = T.ctx_with(res, t, w, max_triangles=small)
    ctx.marching_cubes_region(thr, *b1)
    ctx.marching_cubes_region(thr, *b2)
    got = ctx.triangles()
    assert len(got) == small and T.same_bits(got, both[:small])
    ctx.marching_cubes_region(thr, *b1)                            # a full buffer stays as it is
    assert T.same_bits(ctx.triangles(), both[:small])
    ctx.close()


# ---- 4. the persistent class tables --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 72])
def test_whole_after_region(res):
    """region calls must leave mc_codes / mc_surv fit for the next whole-volume extraction"""
    thr = T.thr_of(res)
    a, b = T.scene_ctx(res), T.scene_ctx(res)
    h = res // 2
    for lo, hi in (((h - 3, 5, 0), (h + 2, res - 9, res)), ((0, 0, h - 9), (res, res, h - 6)), ((11, 13, 9), (20, 17, 44))):
        a.marching_cubes_region(thr, lo, hi)
    assert len(a.triangles()) > 0
    a.clear_triangles()
    a.marching_cubes(thr)
    b.marching_cubes(thr)
    ta, tb = a.triangles(), b.triangles()
    assert len(tb) > 1000 and T.same_bits(ta, tb)
    a.close(); b.close()


@pytest.mark.parametrize("res", [64, 72])
def test_region_after_whole_and_more_fusion(res):
    """the other order: a whole-volume extraction, two more fused frames (new has-negative bricks), then a region -- it must not trust rows the
    whole-volume pass wrote for the older volume -- and a whole-volume extraction again"""
    thr = T.thr_of(res)
    a, b = T.make_ctx(res), T.make_ctx(res)
    T.fuse(a, range(3)); T.fuse(b, range(3))
    a.marching_cubes(thr)
    assert len(a.triangles()) > 1000
    for ctx in (a, b):
        for k in (3, 4):
            assert T.run_frame(ctx, k)[0]
    t, w, _ = T.planes(a)
    tb, wb, _ = T.planes(b)
    assert T.same_bits(t, tb) and T.same_bits(w, wb)
    h = res // 2
    lo, hi = (h - 13, 9, h - 15), (h + 14, h + 9, h + 20)
    a.clear_triangles()
    a.marching_cubes_region(thr, lo, hi)
    got = a.triangles()
    want = T.masked_soup(res, t, w, None, lo, hi, thr)
    assert len(want) > 100 and T.same_bits(got, want)
    a.clear_triangles()
    a.marching_cubes(thr)
    b.marching_cubes(thr)
    assert T.same_bits(a.triangles(), b.triangles())
    a.close(); b.close()


# ---- 5. cost follows the box ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,res", [("scene", 72), ("stress", 64)])
def test_cost_follows_the_box(kind, res):
    """bounds derived from the rule, not measured: a cell reads voxels -1 .. +1, so the class pass reads at most the bricks the box touches widened
    by one brick; the blocks listed are at most the 256-cell blocks of the box (its x range widened to whole bricks)"""
    t, w, c, thr, cap = volume(kind, res, False)
    nb = res // 8
    ctx = T.ctx_with(res, t, w, max_triangles=cap)
    assert ctx.region_work() == (0, 0)
    ctx.marching_cubes(thr)                                        # the whole-volume extraction allocates the scratch: still no region call to report
    assert ctx.region_work() == (0, 0)
    for axis in range(3):
        lo, hi = [0, 0, 0], [res, res, res]
        lo[axis], hi[axis] = 32, 40                                # brick 4: a strip one brick thick
        ctx.clear_triangles()
        ctx.marching_cubes_region(thr, lo, hi)
        bricks, blocks = ctx.region_work()
        assert len(ctx.triangles()) > 0
        assert 0 < bricks <= 3 * nb * nb, (axis, bricks)
        assert 0 < blocks <= (8 * res * res + 255) // 256, (axis, blocks)
    lo = (24, 32, 24) if kind == "stress" else (32, 32, 24)        # one interior brick (the scene's: on the central sphere)
    ctx.clear_triangles()
    ctx.marching_cubes_region(thr, lo, [v + 8 for v in lo])
    bricks, blocks = ctx.region_work()
    assert len(ctx.triangles()) > 0 and 0 < bricks <= 27 and 0 < blocks <= 2
    ctx.marching_cubes_region(thr, (5, 5, 5), (5, 9, 9))           # an empty box: nothing visited
    assert ctx.region_work() == (0, 0)
    ctx.close()


# ---- 6. world coordinates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", [(64, False), (72, True)])
def test_world_flag(res, color):
    ctx = T.scene_ctx(res, color)
    thr = T.thr_of(res)
    d = (8, -16, 24)
    lo, hi = (0, 3, 0), (res - 11, res, res - 7)
    ctx.marching_cubes_region(thr, lo, hi, has_color=color, flags=K.MC_WORLD)      # zero origin: untouched
    zero_world = ctx.triangles()
    ctx.clear_triangles()
    ctx.marching_cubes_region(thr, lo, hi, has_color=color)
    assert len(zero_world) > 100 and T.same_bits(zero_world, ctx.triangles())
    ctx.shift_volume(*d)
    assert ctx.volume_origin() == d
    ctx.clear_triangles()
    ctx.marching_cubes_region(thr, lo, hi, has_color=color)
    plain = ctx.triangles()
    ctx.clear_triangles()
    ctx.marching_cubes_region(thr, lo, hi, has_color=color, flags=K.MC_WORLD)
    world = ctx.triangles()
    assert len(plain) > 100
    assert T.same_bits(world, T.to_world(plain, d, ctx.size / res))
    assert not T.same_bits(world, plain)
    ctx.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ARG, STATE = 1001, 1002
    res = 64
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(res, res, res)
    thr = T.thr_of(res)
    ctx = T.scene_ctx(res)
    lib = ctx.lib
    assert lib.kf_marching_cubes_region(None, 0, thr, lo, hi, 0) == ARG
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, None, hi, 0) == ARG
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, lo, None, 0) == ARG
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, lo, hi, 4) == ARG
    assert lib.kf_marching_cubes_region(ctx.h, 1, thr, lo, hi, 0) == STATE                       # no colour volume
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, lo, hi, K.MC_TO_WORLD_SOUP) == ARG         # the soup is in world coordinates
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, lo, hi, K.MC_WORLD | K.MC_TO_WORLD_SOUP) == STATE   # no soup reserved
    assert lib.kf_set_stream_out(ctx.h, 1, 0, thr) == STATE
    assert lib.kf_clear_world_soup(ctx.h) == STATE and lib.kf_append_world_soup(ctx.h) == STATE
    assert lib.kf_region_work(ctx.h, None) == ARG
    assert ctx.world_soup_count() == (0, 0)
    assert len(ctx.triangles()) == 0                               # nothing was enqueued by any of them
    inv_lo, inv_hi = (C.c_int32 * 3)(9, 9, 9), (C.c_int32 * 3)(30, 4, 30)
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, inv_lo, inv_hi, 0) == 0 and len(ctx.triangles()) == 0      # inverted: a no-op
    ctx.world_soup_reserve(1000)
    assert lib.kf_set_stream_out(ctx.h, 1, 1, thr) == STATE        # colour stream-out without a colour volume
    assert lib.kf_set_stream_out(ctx.h, 1, 0, thr) == 0
    ctx.world_soup_reserve(0)
    assert lib.kf_marching_cubes_region(ctx.h, 0, thr, lo, hi, K.MC_WORLD | K.MC_TO_WORLD_SOUP) == STATE
    ctx.close()
    slab = T.make_ctx(res, slab=(0, 32), halo=8)
    assert slab.lib.kf_marching_cubes_region(slab.h, 0, thr, lo, hi, 0) == ARG
    slab.close()
    none = T.make_ctx(res, max_triangles=0)
    assert none.lib.kf_marching_cubes_region(none.h, 0, thr, lo, hi, 0) == STATE                  # no triangle buffer
    none.close()
