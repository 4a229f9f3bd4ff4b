"""GPU: the map mesh.  kf_marching_cubes_at extracts a box of a VIRTUAL window -- the window as kf_shift_volume would assemble it at another origin, the
brick store's bricks restored -- without moving anything; kf_marching_cubes_map walks a tile lattice fixed in the world with it and so meshes everything
ever fused, once.  Expectations always come from the path that existed before: shift the window there, kf_marching_cubes_region, read the triangles, shift
back.  Everything is compared as bytes, in order.  Shapes, stream and helpers are those of test_gpu_shift.py and test_gpu_brickstore.py: 64 voxels at
2.0 m and 72 at 2.25 m (nine bricks per axis: ragged tables), a 160 x 120 camera, six fused frames of Scene S, colour with the VGA colour camera, a store
of 1024 bricks."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_brickstore as B
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
CASES = B.CASES                                                   # (64, False), (72, False), (64, True)
CAP = B.CAP
MAX_TRIS = 300000
ARG, STATE = 1001, 1002
u32 = B.u32


def thr_of(ctx):
    return 300 * ctx.size / ctx.res


def take(ctx):
    """the triangle buffer's contents; the buffer is left empty"""
    t = ctx.triangles()
    ctx.clear_triangles()
    return t


def at(ctx, frame, lo, hi, color=False, flags=0):
    ctx.clear_triangles()
    ctx.marching_cubes_at(thr_of(ctx), frame, lo, hi, has_color=color, flags=flags)
    work = ctx.region_work()
    return take(ctx), work


def by_shifting(ctx, frame, lo, hi, color=False, flags=0):
    """the expectation: the window moved to `frame`, the region extraction that existed before, the window moved back"""
    o = ctx.volume_origin()
    d = tuple(int(f - x) for f, x in zip(frame, o))
    ctx.shift_volume(*d)
    assert ctx.volume_origin() == tuple(frame)
    ctx.clear_triangles()
    ctx.marching_cubes_region(thr_of(ctx), lo, hi, has_color=color, flags=flags)
    t = take(ctx)
    ctx.shift_volume(*[-x for x in d])
    return t


def boxes(res):
    whole = ((0, 0, 0), (res, res, res))
    strips = [((8, 0, 0), (16, res, res)), ((0, 24, 0), (res, 32, res)), ((0, 0, res - 8), (res, res, res))]      # one brick thick, one per axis
    ragged = ((3, 9, 17), (41, 30, 55))
    empty = ((20, 20, 20), (20, 40, 40))
    return [whole] + strips + [ragged, empty]


def fused(res, color, cap=CAP, **kw):
    ctx = G.make_ctx(res, color, MAX_TRIS, **kw)
    if cap:
        ctx.brick_store_reserve(cap)
    G.fuse(ctx, range(6), color)
    return ctx


def assert_same_frame(ctx, color, what):
    """frame origin == origin: the call IS the region call, box for box, with and without world coordinates"""
    o = ctx.volume_origin()
    n_whole = None
    for flags in (0, K.MC_WORLD):
        for lo, hi in boxes(ctx.res):
            got, _ = at(ctx, o, lo, hi, color, flags)
            ctx.marching_cubes_region(thr_of(ctx), lo, hi, has_color=color, flags=flags)
            want = take(ctx)
            assert G.same_bits(got, want), (what, flags, lo, hi, len(got), len(want))
            if (lo, hi) == boxes(ctx.res)[0]:
                n_whole = len(want)
            if (lo, hi) == boxes(ctx.res)[-1]:
                assert len(got) == 0 and ctx.region_work() == (0, 0)
    assert n_whole > 1000, (what, n_whole)


# ---- 1. the same frame ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,color", CASES)
def test_same_frame_is_the_region_call(res, color):
    ctx = fused(res, color)
    assert_same_frame(ctx, color, "store reserved, nothing in it")
    ctx.close()


@pytest.mark.parametrize("res,color", CASES)
def test_same_frame_without_a_store(res, color):
    """no store reserved is no error; the window stands away from the first cube here, so the world rule adds a non-zero origin on both sides"""
    ctx = fused(res, color, cap=0)
    ctx.shift_volume(8, -8, 16)
    assert_same_frame(ctx, color, "no store")
    ctx.close()


@pytest.mark.parametrize("res,color", CASES)
def test_window_takes_precedence_over_a_stale_store_copy(res, color):
    ctx = fused(res, color)
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
ELSEWHERE = [(32, 0, 0), (24, -24, 16), (0, 0, -24)]              # (0, 0, -24) in place of (0, 0, -16): see test_elsewhere_equals_shifting_there


def half(d):
    """d / 2 rounded to whole bricks (towards zero)"""
    return tuple(int(8 * (abs(x) // 16) * (1 if x >= 0 else -1)) for x in d)


def store_only_cells(ctx, frame):
    """[z, y, x] over the cells of the virtual window at `frame`: the cell's 27-voxel stencil includes a voxel of a brick that only the store holds;
    and the number of bricks of the virtual window that have a source at all, as a [bz, by, bx] mask"""
    res, nb = ctx.res, ctx.res // 8
    o = np.array(ctx.volume_origin()) // 8
    f = np.array(frame) // 8
    held = {tuple(k) for k in ctx.brick_store()[0].tolist()}
    only = np.zeros((nb, nb, nb), bool)
    resolved = np.zeros((nb, nb, nb), bool)
    for bz in range(nb):
        for by in range(nb):
            for bx in range(nb):
                w = f + (bx, by, bz)
                in_window = bool(np.all(w - o >= 0) and np.all(w - o < nb))
                in_store = tuple(int(v) for v in w) in held
                only[bz, by, bx] = in_store and not in_window
                resolved[bz, by, bx] = in_store or in_window
    vox = np.repeat(np.repeat(np.repeat(only, 8, 0), 8, 1), 8, 2)
    p = np.pad(vox, 1)
    cells = np.zeros_like(vox)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                cells |= p[dz:dz + res, dy:dy + res, dx:dx + res]
    return cells, resolved


def cells_of(tris, cell, res):
    """the cell (x, y, z) every triangle of a LOCAL-coordinate extraction came from: its vertices lie on the edges of that cell's cube"""
    pos = tris["v"]["pos"].astype(np.float64)                     # (n, 3 vertices, 3)
    c = np.floor(pos.mean(axis=1) / cell).astype(np.int64)
    return np.clip(c, 0, res - 1)


def widened(lo, hi, nb):
    blo = [max(l >> 3, 0) for l in lo]
    bhi = [min(((h - 1) >> 3) + 1, nb) for h in hi]
    return [max(b - 1, 0) for b in blo], [min(b + 1, nb) for b in bhi]


@pytest.mark.parametrize("d", ELSEWHERE)
@pytest.mark.parametrize("res,color", CASES)
def test_elsewhere_equals_shifting_there(res, color, d):
    """After shift_volume(d): the old place, d itself, half-way, and a far frame; whole and ragged boxes.  `got` is taken first, then the same context
    is shifted to the frame, extracted with the region call and shifted back.  For the old-place frame at least 200 triangles come from cells whose
    stencil reaches into a brick that only the store holds (counted from the expectation): the store's bricks really are meshed.
    The third shift is (0, 0, -24) where the brick store's tests use (0, 0, -16): at 72 voxels the back wall's surface lies in brick layer 6 (voxels 48-55), and
    a shift by two bricks evicts layers 7 and 8 only -- negative voxels behind the wall, but no cell with a triangle reaches them (measured: 0 triangles).
    Three bricks evict the wall itself; the floor of 200 stays."""
    ctx = fused(res, color)
    ctx.shift_volume(*d)
    nb = res // 8
    whole, ragged = boxes(res)[0], boxes(res)[4]
    for frame in [(0, 0, 0), d, half(d), (1024, 0, 0)]:
        for lo, hi in (whole, ragged):
            for flags in (0, K.MC_WORLD):
                cells, resolved = store_only_cells(ctx, frame)     # (every expectation below leaves more bricks in the store)
                got, work = at(ctx, frame, lo, hi, color, flags)
                want = by_shifting(ctx, frame, lo, hi, color, flags)
                assert G.same_bits(got, want), (frame, lo, hi, flags, len(got), len(want))
                wlo, whi = widened(lo, hi, nb)
                n_res = int(np.count_nonzero(resolved[wlo[2]:whi[2], wlo[1]:whi[1], wlo[0]:whi[0]]))
                assert work[0] <= n_res, (frame, lo, hi, work, n_res)
                if frame == (1024, 0, 0):
                    assert len(got) == 0 and work == (0, 0), (lo, hi, work)
                if frame == (0, 0, 0) and (lo, hi) == whole and flags == 0:
                    c = cells_of(want, ctx.size / res, res)
                    n_store = int(np.count_nonzero(cells[c[:, 2], c[:, 1], c[:, 0]]))
                    print(res, color, d, "triangles", len(want), "of them from cells that reach into a store-only brick", n_store)
                    assert n_store >= 200, (d, n_store)
    ctx.close()


# ---- 3. nothing touched ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["icp", "defer", "color"])
def test_nothing_is_touched(variant):
    """Twins with one history; A calls marching_cubes_at and marching_cubes_map between frames, B does not.  Planes, statistics, pose, store, model maps
    at every level, the whole-volume extraction (its class tables hold rows of another frame after A's calls) and four more frames: bit for bit."""
    res, color = 64, variant == "color"
    a, b = G.make_ctx(res, color, MAX_TRIS), G.make_ctx(res, color, MAX_TRIS)
    for ctx in (a, b):
        if variant == "defer":
            ctx.set_defer(1)
        ctx.brick_store_reserve(CAP)
        G.fuse(ctx, range(6), color)
        if variant == "defer":
            assert ctx.fusion_form()["defer"] == 1
        ctx.shift_volume(32, 0, 0)
        G.raycast(ctx, color)
        ctx.marching_cubes(thr_of(ctx), has_color=color)         # the class tables are in the state a whole-volume extraction leaves and trusts
        assert len(take(ctx)) > 500
    for k in (6, 7):                                              # (with deferral: words are pending again when A extracts)
        for ctx in (a, b):
            ok, _ = G.run_frame(ctx, k, color)
            assert ok, k
    got, _ = at(a, (0, 0, 0), (0, 0, 0), (res, res, res), color, K.MC_WORLD)
    assert len(got) > 1000
    a.clear_triangles()
    assert a.marching_cubes_map(thr_of(a), has_color=color) >= 8
    assert len(take(a)) > 1000

    def same_state(what):
        ta, wa, ca = G.planes(a, color)
        tb, wb, cb = G.planes(b, color)
        assert np.array_equal(u32(ta), u32(tb)) and np.array_equal(u32(wa), u32(wb)), what
        if color:
            assert np.array_equal(ca, cb), what
        assert a.stats() == b.stats(), what
        assert np.array_equal(u32(G.pose_of(a)), u32(G.pose_of(b))), what
        assert a.brick_store_count() == b.brick_store_count() and a.volume_origin() == b.volume_origin(), what
        for x, y in zip(B.store_sorted(a), B.store_sorted(b)):
            assert (x is None and y is None) or G.same_bits(x, y), what

    same_state("after the calls")
    G.assert_same_model(a, b, color)
    for ctx in (a, b):
        ctx.marching_cubes(thr_of(ctx), has_color=color)
    ta, tb = take(a), take(b)
    assert len(tb) > 500 and G.same_bits(ta, tb)
    for k in range(8, 12):
        oka, pa = G.run_frame(a, k, color)
        okb, pb = G.run_frame(b, k, color)
        assert oka and okb, k
        assert np.array_equal(u32(pa), u32(pb)), (k, pa, pb)
        if variant == "defer":
            assert a.fusion_form()["defer"] == 1 and b.fusion_form()["defer"] == 1
    same_state("four frames later")
    a.close(); b.close()


# ---- 4. the map ------------------------------------------------------------------------------------------------------------------------------------
def map_of(ctx, color=False):
    ctx.clear_triangles()
    n = ctx.marching_cubes_map(thr_of(ctx), has_color=color)
    return take(ctx), n


@pytest.mark.parametrize("res,color", CASES)
def test_the_map_is_the_same_wherever_the_window_stands(res, color):
    """Walk (32, 0, 0) -> (32, 32, 0) -> (0, 0, 0).  After each step the map equals the concatenation, in tile order, of what shifting a twin to every
    tile's frame and extracting the tile's owned box [8, res - 8) with the region call gives; and the three maps are the same bytes.  With stream-out on
    as well, the world soup after the walk holds more triangles than the map has outside the window: the duplicates the map does not have."""
    ctx, twin = fused(res, color), fused(res, color)
    ctx.world_soup_reserve(MAX_TRIS)
    ctx.set_stream_out(True, thr_of(ctx), has_color=color)
    maps = []
    for d in [(32, 0, 0), (0, 32, 0), (-32, -32, 0)]:
        ctx.shift_volume(*d)
        twin.shift_volume(*d)
        slo, shi = ctx.brick_store_bounds()
        keys = ctx.brick_store()[0]
        assert slo == tuple(keys.min(axis=0)) and shi == tuple(keys.max(axis=0) + 1)
        frames = K.map_tiles(slo, shi, ctx.volume_origin(), res)
        got, n_tiles = map_of(ctx, color)
        assert n_tiles == len(frames)
        want = [by_shifting(twin, tuple(int(v) for v in f), (8, 8, 8), (res - 8, res - 8, res - 8), color, K.MC_WORLD) for f in frames]
        print(res, color, ctx.volume_origin(), "tiles", n_tiles, "with triangles", sum(len(w) > 0 for w in want), "triangles", len(got))
        # at 64 voxels a tile owns 48 cells and Scene S (voxels 16-48 of the first cube) spans tiles; at 72 it owns 56 and the scene lies inside tile 0
        assert sum(len(w) > 0 for w in want) >= (2 if res == 64 else 1)
        assert G.same_bits(got, np.concatenate(want))
        maps.append(got)
    assert len(maps[0]) > 1000 and G.same_bits(maps[0], maps[1]) and G.same_bits(maps[1], maps[2])
    assert ctx.volume_origin() == (0, 0, 0) and ctx.brick_store_count()[1] == 0
    cell = ctx.size / res
    pos = maps[2]["v"]["pos"].astype(np.float64).mean(axis=1)
    off_window = int(np.count_nonzero(np.any((pos < 0) | (pos >= res * cell), axis=1)))
    soup = ctx.world_soup_count()[0]
    print(res, color, "world soup after the walk", soup, "triangles; the map outside the window", off_window, "; the map", len(maps[2]))
    assert soup > off_window
    ctx.close(); twin.close()


# ---- 5. refusals and the off path ----------------------------------------------------------------------------------------------------------------
def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_refusals_touch_nothing():
    res = 64
    ctx = fused(res, False)
    ctx.shift_volume(32, 0, 0)
    thr = thr_of(ctx)
    ctx.marching_cubes_region(thr, (0, 0, 0), (res, res, 32))     # something in the triangle buffer
    tris, (t, w, _), store, counts = ctx.triangles(), G.planes(ctx), B.store_sorted(ctx), ctx.brick_store_count()
    assert len(tris) > 100 and counts[0] >= 20
    lib, h = ctx.lib, ctx.h
    lo, hi, o = i3(0, 0, 0), i3(res, res, res), i3(0, 0, 0)
    assert lib.kf_marching_cubes_at(h, 0, thr, None, lo, hi, 0) == ARG
    assert lib.kf_marching_cubes_at(h, 0, thr, o, None, hi, 0) == ARG
    assert lib.kf_marching_cubes_at(h, 0, thr, o, lo, None, 0) == ARG
    assert lib.kf_marching_cubes_at(h, 0, thr, i3(4, 0, 0), lo, hi, 0) == ARG             # no multiple of 8
    assert lib.kf_marching_cubes_at(h, 0, thr, i3(0, -8, 3), lo, hi, 0) == ARG
    assert lib.kf_marching_cubes_at(h, 0, thr, o, lo, hi, K.MC_TO_WORLD_SOUP) == ARG      # unknown flag bits
    assert lib.kf_marching_cubes_at(h, 0, thr, o, lo, hi, 4 | K.MC_WORLD) == ARG
    assert lib.kf_marching_cubes_at(h, 0, thr, i3(8 * (1 << 20) - 8 * (res // 8) + 8, 0, 0), lo, hi, 0) == ARG     # the frame's last brick would be 2^20
    assert lib.kf_marching_cubes_at(h, 0, thr, i3(0, 0, -8 * (1 << 20) - 8), lo, hi, 0) == ARG
    assert lib.kf_marching_cubes_at(h, 1, thr, o, lo, hi, 0) == STATE                     # colour without a colour plane
    assert lib.kf_marching_cubes_map(h, 1, thr, K.MC_WORLD, None) == STATE
    assert lib.kf_marching_cubes_map(h, 0, thr, 2, None) == ARG
    assert lib.kf_marching_cubes_at(h, 0, thr, o, i3(20, 20, 20), i3(20, 40, 40), 0) == 0  # empty: a no-op
    assert lib.kf_marching_cubes_at(h, 0, thr, o, i3(40, 0, 0), i3(8, 64, 64), 0) == 0     # inverted
    assert ctx.region_work() == (0, 0)
    assert lib.kf_marching_cubes_at(h, 0, thr, i3(8 * (1 << 20) - 8 * (res // 8), 0, 0), lo, hi, 0) == 0   # the last legal frame: nothing there
    assert ctx.region_work() == (0, 0)
    assert G.same_bits(ctx.triangles(), tris)
    t2, w2, _ = G.planes(ctx)
    assert np.array_equal(u32(t2), u32(t)) and np.array_equal(u32(w2), u32(w))
    assert ctx.brick_store_count() == counts
    for x, y in zip(B.store_sorted(ctx), store):
        assert (x is None and y is None) or G.same_bits(x, y)
    ctx.close()
    slab = G.make_ctx(res, False, MAX_TRIS, slab=(0, 32), halo=8)
    assert slab.lib.kf_marching_cubes_at(slab.h, 0, thr, o, lo, hi, 0) == ARG
    assert slab.lib.kf_marching_cubes_map(slab.h, 0, thr, K.MC_WORLD, None) == ARG
    slab.close()
    bare = G.make_ctx(res)                                        # no triangle buffer
    assert bare.lib.kf_marching_cubes_at(bare.h, 0, thr, o, lo, hi, 0) == STATE
    assert bare.lib.kf_marching_cubes_map(bare.h, 0, thr, K.MC_WORLD, None) == STATE
    assert bare.brick_store_bounds() == ((0, 0, 0), (0, 0, 0))   # no store: lo == hi
    bare.brick_store_reserve(16)
    assert bare.brick_store_bounds() == ((0, 0, 0), (0, 0, 0))   # an empty one
    bare.close()
    small = K.Context(K.camera(*G.CAM), 24, 0.75, G.P["volume_max_weight"], levels=3, max_triangles=1000)
    assert small.lib.kf_marching_cubes_map(small.h, 0, thr, K.MC_WORLD, None) == ARG       # a tile owns res - 16 cells: res >= 32
    small.close()


def test_a_small_buffer_clamps_the_map():
    res, cap = 64, 3000
    full, small = fused(res, False), G.make_ctx(res, False, cap)
    small.brick_store_reserve(CAP)
    G.fuse(small, range(6))
    for ctx in (full, small):
        ctx.shift_volume(32, 0, 0)
    want, n = map_of(full)
    got, n2 = map_of(small)
    assert n == n2 and len(want) > cap + 1000
    assert len(got) == cap and G.same_bits(got, want[:cap])       # clamped like the region call: the first `cap` triangles, the count stops there
    full.close(); small.close()


# ---- 6. the host class ------------------------------------------------------------------------------------------------------------------------------
def test_host_class_map_mesh(tmp_path):
    """The walking-camera stream of test_gpu_shift.py with the recentring policy, a brick store and the map mesh on: generateMesh is
    kf_marching_cubes_map on the C ABI, and saveMesh with the device weld writes the mesh kf_weld_mesh makes of that soup."""
    n = 20
    app = H.App(G.H_RES, G.H_SIZE, G.CAM, sdf_trunc=5 * G.H_SIZE / G.H_RES, integrate_dist=3.6, max_triangles=600000)
    app.set_recentre(G.H_DIST)
    app.set_brick_store(4096)
    app.set_map_mesh(True)
    app.set_device_weld(True)
    for k in range(n):
        assert app.process_frame(S.render_depth_mm(G.walk_pose(k, n), G.CAM, G.H_SIZE), k, stamp=float(k)), k
    assert app.volume_origin() != (0, 0, 0)
    # the policy's own shifts are a brick or two and evict only empty layers of this scene (it sits in [0.25, 0.75] of the first cube): one explicit
    # shift by six bricks puts the scene's left wall into the store, so that the map has an off-window part
    assert app.shift_volume(48, 0, 0)
    held, dropped, _ = app.brick_store_count()
    assert held >= 20 and dropped == 0
    n_tris = app.generate_mesh()
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*G.CAM), G.H_RES, G.H_SIZE)
    got = ctx.triangles()
    assert n_tris == len(got) and n_tris > 1000
    want, n_tiles = map_of(ctx)
    print("host class: tiles", n_tiles, "triangles", n_tris, "bricks held", held)
    assert G.same_bits(got, want)
    assert app.generate_mesh() == n_tris                          # generateMesh clears first: the map once, not twice
    ok, nv, nf = app.save_mesh(str(tmp_path / "map.ply"))
    assert ok
    ctx.weld_mesh(False, 1e-4)
    assert (nv, nf) == ctx.mesh_counts()[:2] and nv > 500
    head = open(str(tmp_path / "map.ply"), "rb").read(1000).decode("ascii", "replace")
    assert "element vertex %d" % nv in head and "element face %d" % nf in head
    v = H.app_mesh()["vertices"]
    # world coordinates with no origin added: the scene sits in [0.25, 0.75] * size of the FIRST cube along y
    assert v[:, 1].min() > 0.2 * G.H_SIZE and v[:, 1].max() < 0.8 * G.H_SIZE
    app.close()
