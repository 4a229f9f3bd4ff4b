"""GPU: the distance field of the map.  kf_map_distance_field gives, for every voxel of a box, the exact squared distance in voxels to the nearest site of
the map -- window and, outside it, brick store -- up to a radius, and the class bytes.  The yardstick is tests/map_edt_expect.py (np_classify, np_edt: the
definition in include/hybkf.h restated in numpy), held against the brute-force minimum and scipy by tests/test_map_edt_cpu.py, which also shows that the
analytic sets used here hold every kind of voxel.  Contexts, stream and helpers are those of test_gpu_map_query.py: 64 voxels at 2.0 m, the 160 x 120
camera, 6 fused frames of Scene S, a store of 1024 bricks.  Everything is compared bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import map_edt_expect as E
import map_query_expect as Q
import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_map_query as MQ
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAP = B.CAP
ARG, STATE = 1001, 1002
OCC = 1 << E.OCCUPIED
RES = 64


def assert_field(got, want, what, keys=("dist2", "cls")):
    for k, w in zip(("dist2", "cls"), want):
        if k in keys:
            assert got[k].shape == w.shape and got[k].dtype == w.dtype, (what, k, got[k].shape, w.shape)
            assert np.array_equal(got[k], w), (what, k, int(np.count_nonzero(got[k] != w)))


@functools.lru_cache(maxsize=None)
def analytic_expected(kind, R, lo, dims, level=0.0, mask=OCC):
    return E.expected(E.analytic_map(kind, R, lo, dims), lo, dims, R, level, mask)


# ---- 1. analytic maps in the store ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,R,lo,dims", E.analytic_sets())
def test_analytic_maps(kind, R, lo, dims):
    ctx = MQ.store_only_ctx(RES, False, E.analytic_map(kind, R, lo, dims))
    want = analytic_expected(kind, R, lo, dims)
    assert_field(ctx.map_distance_field(lo, dims, R), want, (kind, R))
    assert (want[0] == R * R).any() and (want[0] == E.FAR).any()
    ctx.close()


def test_empty_store():
    ctx = G.make_ctx(RES, False)
    ctx.brick_store_reserve(CAP)
    ctx.shift_volume(0, 0, -4096)
    assert ctx.brick_store_count()[0] == 0
    got = ctx.map_distance_field(E.BOX_LO, E.BOX_DIMS, 7)
    assert (got["dist2"] == E.FAR).all() and (got["cls"] == E.UNKNOWN).all()
    ctx.close()


# ---- 2. window and store together; deferred weights; no store ------------------------------------------------------------------------------------------------
def straddling_box(d, window, origin):
    """a box of BOX_DIMS across the window's +x face, not brick-aligned, around a store brick beyond the face that holds occupied voxels and whose neighbour
    inside the window does too; returns (lo, dims, that window brick)"""
    face_b = (origin[0] + RES) // 8

    def occupied(k):
        return k in d and bool(np.any((d[k][1] > 0) & (d[k][0] <= 0)))
    cand = [k for k in sorted(d) if k[0] == face_b and k not in window and occupied(k) and (face_b - 1, k[1], k[2]) in window and occupied((face_b - 1, k[1], k[2]))]
    assert cand, "no surface across the window's +x face"
    k = cand[len(cand) // 2]
    return (8 * face_b - 19, 8 * k[1] - 7, 8 * k[2] - 5), E.BOX_DIMS, (face_b - 1, k[1], k[2])


def both_sources(d, lo, dims, R, origin):
    """occupied voxels of the widened box inside the window's x range and beyond it"""
    c = E.dense_classes(d, lo, dims, R, 0.0)
    face = origin[0] + RES - (lo[0] - R)
    return int(np.count_nonzero(c[:, :, :face] == E.OCCUPIED)), int(np.count_nonzero(c[:, :, face:] == E.OCCUPIED))


def test_window_and_store():
    R = 7
    ctx = MQ.mixed_ctx(RES, False)
    origin = ctx.volume_origin()
    d, window = MQ.map_dict(ctx, False)
    lo, dims, wkey = straddling_box(d, window, origin)
    n_win, n_store = both_sources(d, lo, dims, R, origin)
    print("occupied voxels of the widened box: window", n_win, "store", n_store)
    assert n_win >= 16 and n_store >= 16
    want = E.expected(d, lo, dims, R)
    assert (want[0] == 0).any() and (want[0] > 0).any()
    assert_field(ctx.map_distance_field(lo, dims, R), want, "window and store")
    # a stale brick in the store under a key inside the window: the window's copy wins
    ctx.write_brick_store(np.array([wkey], np.int32), np.full((1, 8, 8, 8), -1, f32), np.ones((1, 8, 8, 8), f32), None)
    assert not np.all(d[wkey][0] == -1)
    assert_field(ctx.map_distance_field(lo, dims, R), want, "a stale brick in the store")
    # the same map with the window elsewhere: captured, then shifted away
    ctx.brick_store_capture()
    ctx.shift_volume(0, 0, -4096)
    assert_field(ctx.map_distance_field(lo, dims, R), want, "captured, the window elsewhere")
    ctx.close()


@pytest.mark.parametrize("max_weight", [2.0, 128.0])
def test_deferred_weights(max_weight):
    """set_defer(1): the window's stored weights lag behind, the deferred-weight words carry the rest (max_weight 2: saturated quarters).  The field is asked
    for while the words are live -- nothing has read the volume out since the last deferred fusion pass -- and must class by the TRUE weights, those of the
    read-out taken afterwards, and leave the words as they are (test_bystander).  A word is only ever set on a quarter brick whose 128 stored weights are all
    >= 1 (integrate.hip, "DEFER"), so "stored weight 0, true weight > 0" does not occur and no class can depend on the word: what this case pins is the call
    in the live state, on a box that the three deferred frames changed"""
    R = 7
    ctx = MQ.mixed_ctx(RES, False, defer=1, max_weight=max_weight)
    origin = ctx.volume_origin()
    d0, window = MQ.map_dict(ctx, False)
    lo, dims, _ = straddling_box(d0, window, origin)
    MQ.fuse_on(ctx, (6, 7, 8))
    assert ctx.fusion_form()["defer"] == 1
    got = ctx.map_distance_field(lo, dims, R)
    d, _ = MQ.map_dict(ctx, False)                                # (after the call)
    want = E.expected(d, lo, dims, R)
    before = E.expected(d0, lo, dims, R)[1]
    # voxels of the box that the three frames fused with deferral on observed for the first time
    newly = int(np.count_nonzero((before == E.UNKNOWN) & (want[1] != E.UNKNOWN)))
    print("voxels of the box observed by the deferred frames alone:", newly)
    assert newly >= 1
    assert_field(got, want, ("deferred", max_weight))
    ctx.close()


def test_no_store_reserved():
    """the window alone is the map; everything outside it reads unknown"""
    R = 7
    ctx = MQ.mixed_ctx(RES, False, store=False)
    origin = ctx.volume_origin()
    d, window = MQ.map_dict(ctx, False, store=False)
    seen = [k for k in sorted(window) if k[0] == (origin[0] + RES) // 8 - 1 and np.any((d[k][1] > 0) & (d[k][0] <= 0))]
    assert seen
    k = seen[len(seen) // 2]
    lo, dims = (8 * k[0] - 11, 8 * k[1] - 7, 8 * k[2] - 5), E.BOX_DIMS
    for mask in (OCC, OCC | 1 << E.UNKNOWN):
        want = E.expected(d, lo, dims, R, 0.0, mask)
        assert (want[1][:, :, 30:] == E.UNKNOWN).all() and (want[1] == E.OCCUPIED).any()
        assert_field(ctx.map_distance_field(lo, dims, R, 0.0, mask), want, ("no store", mask))
    ctx.close()


# ---- 4. far keys -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "plane", "sphere"])
def test_far_keys(kind):
    R = 7
    ctx = MQ.store_only_ctx(RES, False, Q.shifted(E.analytic_map(kind, R), Q.FAR))
    assert_field(ctx.map_distance_field(E.moved_lo(E.BOX_LO, Q.FAR), E.BOX_DIMS, R), analytic_expected(kind, R, E.BOX_LO, E.BOX_DIMS), ("far keys", kind))
    ctx.close()


def test_halo_beyond_the_key_range():
    """a box that ends at the key range's last voxel: what the radius reaches beyond reads unknown -- a wall of sites where unknown is an obstacle, nothing
    where it is not; and a box that itself leaves the range is refused"""
    R, top = 7, 1 << 23
    bricks = {(bx, by, bz): (np.ones((8, 8, 8), f32), np.ones((8, 8, 8), f32), None) for bx in range((1 << 20) - 4, 1 << 20) for by in range(-3, 4) for bz in range(-3, 4)}
    site = np.array([top - 9, 3, 2])
    E._put_site(bricks, site)
    ctx = MQ.store_only_ctx(RES, False, bricks)
    lo, dims = (top - 12, -5, -4), (12, 11, 9)
    for mask in (OCC, OCC | 1 << E.UNKNOWN, 1 << E.UNKNOWN):
        want = E.expected(bricks, lo, dims, R, 0.0, mask)
        if mask & 1:
            x = np.arange(12)
            assert np.array_equal(want[0][8, 0, 6:], ((12 - x) ** 2)[6:])   # the wall at x = 2^23, seen from a row further than R from the site
        assert_field(ctx.map_distance_field(lo, dims, R, 0.0, mask), want, ("key range", mask))
    d, c = np.full(12 * 11 * 9, 7, np.uint16), np.full(12 * 11 * 9, 7, np.uint8)
    for bad in ((top - 11, -5, -4), (-top - 1, -5, -4), (0, top - 10, 0)):
        assert ctx.lib.kf_map_distance_field(ctx.h, (C.c_int32 * 3)(*bad), (C.c_uint32 * 3)(*dims), R, C.c_float(0), OCC, K._p(d), K._p(c)) == ARG, bad
    assert (d == 7).all() and (c == 7).all()
    ctx.close()


# ---- 5. site masks, 6. level -----------------------------------------------------------------------------------------------------------------------------------
def test_site_masks():
    R, kind = 7, "sphere"
    ctx = MQ.store_only_ctx(RES, False, E.analytic_map(kind, R))
    for mask in range(1, 8):
        want = analytic_expected(kind, R, E.BOX_LO, E.BOX_DIMS, 0.0, mask)
        got = ctx.map_distance_field(E.BOX_LO, E.BOX_DIMS, R, 0.0, mask)
        assert_field(got, want, ("mask", mask))
        if mask == 7:
            assert (got["dist2"] == 0).all()
        else:
            assert (got["dist2"] != 0).any() and (got["dist2"] == 0).any()
    beside = (500, 500, 500)                                      # a box beside the map: nobody holds a voxel within its radius
    assert (ctx.map_distance_field(beside, E.BOX_DIMS, R, 0.0, OCC | 1 << E.UNKNOWN)["dist2"] == 0).all()
    got = ctx.map_distance_field(beside, E.BOX_DIMS, R, 0.0, OCC)
    assert (got["dist2"] == E.FAR).all() and (got["cls"] == E.UNKNOWN).all()
    ctx.close()


def test_level():
    """the plane map moved so that the surface itself cuts the box (in the "plane" set only its far corner does, where the tsdf is clamped to -1): a level of
    +-0.25 is one voxel of the band of four"""
    R = 7
    bricks = {k: (t, w, None) for k, (t, w, c) in Q.shifted(Q.plane_map(), (-4, -2, -12)).items()}
    ctx = MQ.store_only_ctx(RES, False, bricks)
    fields = []
    for level in (0.0, 0.25, -0.25):
        want = E.expected(bricks, E.BOX_LO, E.BOX_DIMS, R, level)
        assert_field(ctx.map_distance_field(E.BOX_LO, E.BOX_DIMS, R, level), want, ("level", level))
        fields.append(want)
    assert np.count_nonzero(fields[1][1] == E.OCCUPIED) > np.count_nonzero(fields[0][1] == E.OCCUPIED) > np.count_nonzero(fields[2][1] == E.OCCUPIED)
    ctx.close()


# ---- 7. sub-box ------------------------------------------------------------------------------------------------------------------------------------------------
def test_sub_box():
    kind = "sphere"
    for R in (7, 37):
        ctx = MQ.store_only_ctx(RES, False, E.analytic_map(kind, R))
        outer = ctx.map_distance_field(E.BOX_LO, E.BOX_DIMS, R)
        off, n = (23, 3, 2), (15, 19, 13)
        inner = ctx.map_distance_field(tuple(l + o for l, o in zip(E.BOX_LO, off)), n, R)
        for k in ("dist2", "cls"):
            assert np.array_equal(inner[k], outer[k][off[2]:off[2] + n[2], off[1]:off[1] + n[1], off[0]:off[0] + n[0]]), (R, k)
        assert (inner["dist2"] == 0).any() and (inner["dist2"] > 49).any()
        ctx.close()


# ---- 9. device form against host form ----------------------------------------------------------------------------------------------------------------------------
def test_device_form_and_null_outputs():
    import torch
    R, kind, lo, dims = 7, "sphere", E.BOX_LO, E.BOX_DIMS
    ctx = MQ.store_only_ctx(RES, False, E.analytic_map(kind, R))
    want = analytic_expected(kind, R, lo, dims)
    n, guard = int(np.prod(dims)), 64
    dev = torch.device("cuda")
    d2 = torch.full((n + guard,), 0x0707, dtype=torch.int16, device=dev)
    cls = torch.full((n + guard,), 7, dtype=torch.uint8, device=dev)

    def check(ask_d, ask_c, what):
        d2.fill_(0x0707)
        cls.fill_(7)
        torch.cuda.synchronize()
        ctx.map_distance_field_device(lo, dims, R, 0.0, OCC, d2.data_ptr() if ask_d else None, cls.data_ptr() if ask_c else None)
        ctx.sync()
        hd, hc = d2.cpu().numpy().view(np.uint16), cls.cpu().numpy()
        assert (hd[n:] == 0x0707).all() and (hc[n:] == 7).all(), what                     # the guard past the outputs' ends
        assert np.array_equal(hd[:n].reshape(want[0].shape), want[0]) if ask_d else (hd == 0x0707).all(), what
        assert np.array_equal(hc[:n].reshape(want[1].shape), want[1]) if ask_c else (hc == 7).all(), what
    check(True, True, "both")
    check(True, False, "dist2 alone")
    check(False, True, "cls alone")
    check(False, False, "neither")
    assert_field(ctx.map_distance_field(lo, dims, R, want=("dist2",)), want, "host, dist2 alone", ("dist2",))
    assert_field(ctx.map_distance_field(lo, dims, R, want=("cls",)), want, "host, cls alone", ("cls",))
    ctx.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = K.load()
    p = K._p
    ctx = MQ.store_only_ctx(RES, False, E.analytic_map("single", 7))
    d, c = np.full(8 * 8 * 8, 7, np.uint16), np.full(8 * 8 * 8, 7, np.uint8)
    top = 1 << 23

    def i3(v):
        return (C.c_int32 * 3)(*v)

    def u3(v):
        return (C.c_uint32 * 3)(*v)
    ok = dict(lo=i3((0, 0, 0)), dims=u3((8, 8, 8)), radius=3, level=0.0, mask=OCC)
    bad = [dict(lo=None), dict(dims=None), dict(dims=u3((0, 8, 8))), dict(dims=u3((8, 0, 8))), dict(dims=u3((8, 8, 0))), dict(lo=i3((-top - 1, 0, 0))),
           dict(lo=i3((0, top - 7, 0))), dict(lo=i3((0, 0, top))), dict(radius=0), dict(radius=256), dict(mask=0), dict(mask=8), dict(level=float("nan")),
           dict(dims=u3((1024, 1024, 1024)), radius=1), dict(lo=i3((0, 0, 0)), dims=u3((1, 1, (1 << 24))), radius=255)]
    for fn in (lib.kf_map_distance_field, lib.kf_map_distance_field_device):
        for change in bad:
            a = dict(ok, **change)
            assert fn(ctx.h, a["lo"], a["dims"], a["radius"], C.c_float(a["level"]), a["mask"], p(d), p(c)) == ARG, change
    assert (d == 7).all() and (c == 7).all()
    assert lib.kf_map_distance_field(ctx.h, ok["lo"], ok["dims"], 3, C.c_float(0.0), OCC, None, None) == 0           # nothing asked for: nothing done
    assert lib.kf_map_distance_field(ctx.h, ok["lo"], ok["dims"], 3, C.c_float(0.0), OCC, p(d), p(c)) == 0 and not (d == 7).all() and not (c == 7).all()
    ctx.close()
    d[:], c[:] = 7, 7
    slab = K.Context(K.camera(*G.CAM), RES, 2.0, G.P["volume_max_weight"], levels=3, slab=(0, 32))
    for fn in (lib.kf_map_distance_field, lib.kf_map_distance_field_device):
        assert fn(slab.h, ok["lo"], ok["dims"], 3, C.c_float(0.0), OCC, p(d), p(c)) == STATE
    assert (d == 7).all() and (c == 7).all()
    slab.close()


# ---- 11. bystander -----------------------------------------------------------------------------------------------------------------------------------------------
def mesh_ctx():
    """MQ.mixed_ctx(64, False, defer=1) with a triangle buffer"""
    ctx = G.make_ctx(RES, False, max_triangles=300000)
    ctx.set_defer(1)
    ctx.brick_store_reserve(CAP)
    G.fuse(ctx, range(6))
    ctx.brick_store_capture()
    ctx.shift_volume(*MQ.SHIFT)
    G.raycast(ctx)
    return ctx


def map_mesh(ctx):
    ctx.clear_triangles()
    ctx.marching_cubes_map(300 * ctx.size / ctx.res)
    return ctx.triangles().tobytes()


def test_bystander():
    """the digest of volume, store, pose and model maps is the same before and after the calls; a map mesh extracted between two calls is still in the
    triangle buffer, byte for byte, after the second; and a context that asked BEFORE anything read the deferred-weight words out goes on exactly as its twin
    that never asked: the same next frame, the same map mesh"""
    R = 7
    a, b = mesh_ctx(), mesh_ctx()
    d, window = MQ.map_dict(b, False)                             # placed on the twin: nothing has read A's volume out
    lo, dims, _ = straddling_box(d, window, b.volume_origin())
    MQ.fuse_on(a, (6, 7))
    MQ.fuse_on(b, (6, 7))                                         # live words on both
    first = a.map_distance_field(lo, dims, R)
    assert (first["dist2"] == 0).any() and (first["cls"] == E.FREE).any()
    before = MQ.digest(a, False)
    mesh = map_mesh(a)
    assert len(mesh) > 1000 * 36
    second = a.map_distance_field(lo, dims, 37, 0.0, OCC | 1 << E.UNKNOWN)
    assert a.triangles().tobytes() == mesh                        # the extraction's buffers are not the field's scratch
    third = a.map_distance_field(lo, dims, R)
    assert np.array_equal(third["dist2"], first["dist2"]) and np.array_equal(third["cls"], first["cls"]) and (second["dist2"] != E.FAR).any()
    assert MQ.digest(a, False) == before
    assert MQ.digest(b, False) == before
    for ctx in (a, b):
        G.run_frame(ctx, 8)
    assert MQ.digest(a, False) == MQ.digest(b, False)
    assert map_mesh(a) == map_mesh(b)
    a.close()
    b.close()


# ---- 12. the application in metres, the tiled host class, the tool -------------------------------------------------------------------------------------------------
def test_application_in_metres_and_the_tool(tmp_path):
    res, size, cam = RES, G.SIZES[RES], G.CAM
    cell = f32(size) / f32(res)
    path, out = str(tmp_path / "session.hkfmap"), str(tmp_path / "esdf.npz")
    app = M.make_app(res, size, cam, False)
    try:
        app.set_brick_store(CAP)
        for k in range(6):
            assert M.app_frame(app, k, size, cam, False), k
            if k == 2:
                assert app.shift_volume(32, 0, 0)
        assert app.save_map(path)
    finally:
        app.close()
    app = M.make_app(res, size, cam, False)
    try:
        assert app.load_map(path)
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), res, size)
        lo_vox, dims = (-10, 22, 30), (130, 20, 10)               # across the window's -x face at 32; 130 voxels: two tiles of the host class
        lo_m = [float(v) * float(cell) for v in lo_vox]           # (cell is 1 / 32: exact)
        hi_m = [float(v + n) * float(cell) for v, n in zip(lo_vox, dims)]
        dist, cls, radius = app.distance_field(lo_m, hi_m, 0.1)
        assert radius == 3 and app.distance_field_box(lo_m, hi_m, 0.1) == (lo_vox, dims, 3) and dist.shape == (10, 20, 130) and dist.dtype == f32
        ref = ctx.map_distance_field(lo_vox, dims, radius)        # one untiled call
        want = np.where(ref["dist2"] == E.FAR, f32(np.inf), np.sqrt(ref["dist2"].astype(f32)) * cell).astype(f32)
        assert np.array_equal(dist.view(np.uint32), want.view(np.uint32)) and np.array_equal(cls, ref["cls"])
        assert np.isinf(dist).any() and (dist == 0).any() and (cls == E.FREE).any()
        both = OCC | 1 << E.UNKNOWN                               # unknown as an obstacle: the second tile, beyond everything observed, is all sites
        dist_u, cls_u, _ = app.distance_field(lo_m, hi_m, 0.1, 0.0, both)
        ref_u = ctx.map_distance_field(lo_vox, dims, radius, 0.0, both)
        assert np.array_equal(dist_u.view(np.uint32), np.where(ref_u["dist2"] == E.FAR, f32(np.inf), np.sqrt(ref_u["dist2"].astype(f32)) * cell).astype(f32).view(np.uint32))
        assert np.array_equal(cls_u, cls) and (dist_u[:, :, 128:] == 0).all() and (dist_u > 0).any()
        d, window = MQ.map_dict(ctx, False)
        assert_field(ref, E.expected(d, lo_vox, dims, radius), "the loaded map")
        assert app.distance_field(lo_m, hi_m, 1e9)[2] == 255 and app.distance_field(lo_m, hi_m, 0.0)[2] == 1       # the clamp, reported back
        with pytest.raises(K.KfError):
            app.distance_field(hi_m, lo_m, 0.1)                   # an empty box
        with pytest.raises(K.KfError):
            app.distance_field([-np.inf] * 3, [np.inf] * 3, 0.1)  # 2^24 voxels per axis: refused before anything is sized
        with pytest.raises(K.KfError):
            app.distance_field(lo_m, [hi_m[0], hi_m[1], 1e6], 0.1)        # 130 x 20 x 2^23: above the host classes' bound
    finally:
        app.close()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_esdf.py"), path, out, "--box"] + [repr(v) for v in lo_m + hi_m] + ["--radius", "0.1"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    z = np.load(out)
    assert np.array_equal(z["dist"].view(np.uint32), dist.view(np.uint32)) and np.array_equal(z["cls"], cls)
    assert tuple(z["lo_vox"]) == lo_vox and f32(z["cell"]) == cell


def test_slab_application_refuses():
    sl = H.SlabsApp(RES, 2.0, G.CAM, [0, 32, 64])
    try:
        with pytest.raises(K.KfError):
            sl.distance_field((0, 0, 0), (1, 1, 1), 0.5)
    finally:
        sl.close()
