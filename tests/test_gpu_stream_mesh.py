"""GPU: streaming the departing surface into the world soup.  With stream-out on, kf_shift_volume first extracts every cell whose 27 voxels
include a voxel that is about to leave, in world coordinates, into a second triangle buffer that outlives the window; the host classes hand out
[world soup, current window] as one mesh.  Expectations are stated with region extractions on a twin context that never shifts (pinned to the
whole-volume extraction by test_gpu_mc_region.py) and with the masked-volume construction of stream_common.py.  Bit for bit unless said."""
import numpy as np
import pytest

import stream_common as T
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
f32 = np.float32
SOUP = 200000


def strips(d, R):
    """the rule, by hand: per axis the departing strip; the boxes are the x strip, the y strip without it, the z strip without both"""
    strip, keep = [], []
    for k in range(3):
        if d[k] > 0:
            s = (0, min(d[k] + 1, R)); kp = (s[1], R)
        elif d[k] < 0:
            s = (max(R + d[k] - 1, 0), R); kp = (0, s[0])
        else:
            s = (0, 0); kp = (0, R)
        strip.append(s); keep.append(kp)
    out = []
    for k in range(3):
        rng = [keep[j] if j < k else (strip[j] if j == k else (0, R)) for j in range(3)]
        if all(a < b for a, b in rng):
            out.append((tuple(r[0] for r in rng), tuple(r[1] for r in rng)))
    return out


def twin_world_soup(ctx, boxes, thr, color):
    """the boxes' region soups, in order, in world coordinates, in the twin's triangle buffer"""
    ctx.clear_triangles()
    for lo, hi in boxes:
        ctx.marching_cubes_region(thr, lo, hi, has_color=color, flags=K.MC_WORLD)
    return ctx.triangles()


# ---- 8. one shift --------------------------------------------------------------------------------------------------------------------------
# (resolution, shift, an earlier shift without stream-out, colour).  The scene fills [0.25, 0.75] of the cube, so the earlier shift brings its surfaces
# -- the back wall, the central sphere -- into every strip that is about to leave, and makes the origin non-zero when the stream begins.
ONE = [(64, (8, 0, 0), (16, 0, 0), False), (72, (-8, 0, 0), (-16, 0, 0), False), (64, (0, 16, 0), (0, 8, 0), False), (72, (0, -16, 0), (8, -8, 0), False),
       (64, (0, 0, 24), None, False), (72, (0, 0, -16), (0, 0, -8), False), (64, (16, -8, 24), (16, -16, 0), False), (72, (-8, 16, -16), (-16, 8, -8), True),
       (64, (64, 0, 0), None, False), (72, (0, -80, 8), (0, 8, 0), False)]


@pytest.mark.parametrize("res,d,pre,color", ONE)
def test_one_shift_streams_the_departing_cells(res, d, pre, color):
    thr = T.thr_of(res)
    a, b = T.scene_ctx(res, color), T.scene_ctx(res, color)
    if pre:                                                        # an earlier shift without stream-out: the origin is not zero when the stream begins
        a.shift_volume(*pre); b.shift_volume(*pre)
    a.world_soup_reserve(SOUP)
    a.set_stream_out(True, thr, color)
    boxes = strips(d, res)
    if d == (8, 0, 0):
        assert boxes == [((0, 0, 0), (9, res, res))]               # the cells x < 9
    if abs(d[0]) >= res or abs(d[1]) >= res:
        assert boxes == [((0, 0, 0), (res, res, res))]             # everything is streamed
    assert H.departing_boxes(d, res) == boxes
    for box in boxes:
        assert len(twin_world_soup(b, [box], thr, color)) > 0, box          # every box has surface in it
    want = twin_world_soup(b, boxes, thr, color)
    a.shift_volume(*d)
    n, dropped = a.world_soup_count()
    got = a.world_soup()
    print("res %d shift %s: %d boxes, %d triangles streamed" % (res, d, len(boxes), n))
    assert n == len(want) > 0 and dropped == 0
    assert T.same_bits(got, want)
    assert len(a.triangles()) == 0                                 # the triangle buffer is not touched
    a.shift_volume(0, 0, 0)                                        # no shift: nothing streamed
    assert a.world_soup_count() == (n, 0)
    a.append_world_soup()
    assert T.same_bits(a.triangles(), want)
    a.clear_world_soup()
    assert a.world_soup_count() == (0, 0)
    a.close(); b.close()


# ---- 9. nothing lost, nothing doubled ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 72])
def test_nothing_lost_nothing_doubled(res):
    """After a shift by +16 along x the soup holds cells [0, 17) of the old window and the new window holds the old cells [17, res): cell 16 becomes
    cell 0, which can never be extracted again, cell 17 keeps its 27 voxels.  Expected sets by the masked-volume construction on the UNSHIFTED
    planes, E1 (cells < 17) and E2 (cells >= 17): together they are the whole soup of the unshifted volume.  The soup is E1 bit for bit.  The
    window part is extracted at other coordinates (p - 0.5 m, then + 0.5 m), so against E2 it is compared element by element: same count, same
    order, same colours, positions within 2e-6 m -- each position is a chain of at most four fp32 roundings below 4 m (ulp 2^-22 = 2.4e-7) --
    and bit for bit against the whole-volume extraction of the numpy-shifted planes moved to world coordinates in numpy."""
    thr, cell, d = T.thr_of(res), 1.0 / 32, (16, 0, 0)
    t, w = (T.np_shift(p, (8, 0, 0)) for p in T.fused(res)[:2])    # the scene 8 voxels nearer the face that leaves: the back wall spans cells 8 .. 40
    b = T.ctx_with(res, t, w)
    b.marching_cubes(thr)
    whole = b.triangles()
    b.close()
    e1 = T.masked_soup(res, t, w, None, (0, 0, 0), (17, res, res), thr)
    e2 = T.masked_soup(res, t, w, None, (17, 0, 0), (res, res, res), thr)
    assert len(e1) > 0 and len(e2) > 0 and len(e1) + len(e2) == len(whole)
    assert np.array_equal(T.sorted_words(np.concatenate([e1, e2])), T.sorted_words(whole))
    a = T.ctx_with(res, t, w)
    a.world_soup_reserve(SOUP)
    a.set_stream_out(True, thr)
    a.shift_volume(*d)
    soup = a.world_soup()
    a.marching_cubes_region(thr, (0, 0, 0), (res, res, res), flags=K.MC_WORLD)
    window = a.triangles()
    a.close()
    assert T.same_bits(soup, e1)
    s = T.ctx_with(res, T.np_shift(t, d), T.np_shift(w, d))
    s.marching_cubes(thr)
    assert T.same_bits(window, T.to_world(s.triangles(), d, cell))
    s.close()
    assert len(window) == len(e2)
    assert np.max(np.abs(window["v"]["pos"] - e2["v"]["pos"])) <= 2e-6
    assert T.same_bits(window["v"]["color"], e2["v"]["color"])


# ---- 10. the stream is a bystander ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,d,color", [(64, (16, -8, 24), False), (72, (8, -24, 8), True)])
def test_volume_pose_and_frames_untouched(res, d, color):
    thr = T.thr_of(res)
    a, b = T.make_ctx(res, color), T.make_ctx(res, color)
    T.fuse(a, range(5), color); T.fuse(b, range(5), color)
    a.world_soup_reserve(SOUP)
    a.set_stream_out(True, thr, color)
    a.shift_volume(*d); b.shift_volume(*d)
    assert a.world_soup_count()[0] > 0 and b.world_soup_count() == (0, 0)
    for x, y in zip(T.planes(a, color), T.planes(b, color)):
        assert (x is None and y is None) or T.same_bits(x, y)
    assert T.same_bits(a.track_result()[1], b.track_result()[1]) and a.volume_origin() == b.volume_origin() == d
    for ctx in (a, b):
        T.raycast(ctx, color)
        ctx.downsample(True)
    for level in range(3):
        for m in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
            assert T.same_bits(a.download_map(m, level), b.download_map(m, level)), (m, level)
    for k in (5, 6):
        oka, pa = T.run_frame(a, k, color)
        okb, pb = T.run_frame(b, k, color)
        assert oka == okb and T.same_bits(pa, pb), k
    for x, y in zip(T.planes(a, color), T.planes(b, color)):
        assert (x is None and y is None) or T.same_bits(x, y)
    a.close(); b.close()


# ---- 11. overflow --------------------------------------------------------------------------------------------------------------------------
def test_overflow_clamps_and_counts_what_was_dropped():
    res, d = 64, (24, 0, 8)
    thr = T.thr_of(res)
    a, b = T.scene_ctx(res), T.scene_ctx(res)
    a.shift_volume(0, 0, 16); b.shift_volume(0, 0, 16)             # the sphere into the z strip, the back wall is in the x strip
    want = twin_world_soup(b, strips(d, res), thr, False)
    first_box = twin_world_soup(b, strips(d, res)[:1], thr, False)
    assert len(want) > len(first_box) > 400
    cap = len(first_box) - 150                                     # smaller than the first strip: the second box finds the soup full
    a.world_soup_reserve(cap)
    a.set_stream_out(True, thr)
    a.shift_volume(*d)
    assert a.world_soup_count() == (cap, len(want) - cap)
    assert T.same_bits(a.world_soup(), want[:cap])
    a.shift_volume(0, 0, 8)                                        # still full: everything of the next shift is dropped, the prefix stays
    n, dropped = a.world_soup_count()
    assert n == cap and dropped > len(want) - cap
    assert T.same_bits(a.world_soup(), want[:cap])
    a.clear_world_soup()
    assert a.world_soup_count() == (0, 0)
    a.close(); b.close()


# ---- 12. the host classes ------------------------------------------------------------------------------------------------------------------
H_RES, H_SIZE, H_DIST = 128, 4.0, 0.35
SCENE_DX = 0.8        # the scene stands 0.8 m to the left of where Scene S has it: its back wall (z = 3 m) begins at x = 0.2 m, inside the strips that leave


def walk_pose(k, n):
    """Scene S's 2 cm circle plus 0.75 m along x over n frames, as the camera sees the displaced scene"""
    p = S.trajectory_pose(k, H_SIZE)
    p[0, 3] += SCENE_DX + 0.75 * k / (n - 1)
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_mesh(got, want):
    for k in ("faces", "vertices", "normals"):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k


def test_host_classes_stream_the_mesh(tmp_path):
    n = 20
    app = H.App(H_RES, H_SIZE, T.CAM, sdf_trunc=5 * H_SIZE / H_RES, integrate_dist=3.6, max_triangles=400000)
    app.set_recentre(H_DIST)
    app.set_stream_mesh(SOUP)
    assert app.world_soup_count() == 0
    for k in range(n):
        assert app.process_frame(S.render_depth_mm(walk_pose(k, n), T.CAM, H_SIZE), k)
    o = app.volume_origin()
    assert o[0] >= 8 and o[0] % 8 == 0                             # the window followed the camera
    streamed = app.world_soup_count()
    assert streamed > 0
    ntri = app.generate_mesh()
    assert ntri > streamed
    assert app.generate_mesh() == ntri                             # generateMesh rebuilds [soup, window]: it does not append to itself
    ok, nv, nf = app.save_mesh(str(tmp_path / "host.ply"))
    assert ok and nv > 500
    host = H.app_mesh()
    cell = H_SIZE / H_RES
    v = host["vertices"]
    assert v[:, 0].min() < o[0] * cell - 2 * cell                  # surface that the window has left behind ...
    assert v[:, 0].min() > 0.25 * H_SIZE - SCENE_DX - 0.1          # ... where the scene has it: the back wall begins at x = 0.2 m (world)
    assert v[:, 0].max() > o[0] * cell + 1.0                       # ... and the current window, in the same coordinates, once:
    assert v[:, 0].max() < 0.75 * H_SIZE - SCENE_DX + 0.1          # the right wall stands at x = 2.2 m
    app.set_device_weld(True)
    ok, nv2, nf2 = app.save_mesh(str(tmp_path / "device.ply"))
    assert ok and (nv2, nf2) == (nv, nf)
    same_mesh(H.app_mesh(), host)
    assert open(str(tmp_path / "host.ply"), "rb").read() == open(str(tmp_path / "device.ply"), "rb").read()
    app.close()


def test_host_classes_streaming_off_is_the_old_path(tmp_path):
    """nStreamMeshTriangles = 0: generateMesh + saveMesh through the entry points that existed before -- kf_marching_cubes, the host weld, the origin
    added once -- on a window that has moved"""
    size, res = 2.0, 64
    app = H.App(res, size, T.CAM, sdf_trunc=5 * size / res, integrate_dist=T.GATE, max_triangles=T.MAX_TRI)
    for k in range(4):
        assert app.process_frame(T.frame(k, size), k)
    assert app.shift_volume(8, -8, 16)
    assert app.world_soup_count() == 0
    ntri = app.generate_mesh()
    ok, nv, nf = app.save_mesh(str(tmp_path / "off.ply"))
    assert ok and ntri > 1000
    got = H.app_mesh()
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*T.CAM), res, size)
    soup = ctx.triangles()
    ctx.clear_triangles()
    ctx.marching_cubes(T.thr_of(res))
    assert T.same_bits(ctx.triangles(), soup)
    want = H.mesh_from_soup(soup, False)
    off = np.array([f32(x) * f32(size / res) for x in (8, -8, 16)], f32)
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"] + off)) and np.array_equal(got["faces"], want["faces"])
    app.close()
