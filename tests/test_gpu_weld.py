"""The device weld (csrc/weld.hip: kf_write_triangles / kf_weld_mesh / kf_mesh_counts / kf_read_mesh) against the reference's own
ml::MeshData (tests/golden/mesh_*.npz, made by the reference's classes) and against the host weld those fixtures pin
(host_app.mesh_from_soup, tests/test_mesh_weld.py).  Every comparison is uint32-view equality for floats and plain equality for
indices: the weld has no tolerance anywhere."""
import os

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S
from test_mesh_weld import _ply_mask_alpha

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["mesh_s32", "mesh_s64", "mesh_s64_color", "mesh_stress"]
P = S.STOCK
SMALL_CAM = (160, 120, 79.5, 59.5, 131.25, 131.25)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_mesh(got, want, colors=True):
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"])
    assert got["vertices"].shape == want["vertices"].shape and np.array_equal(bits(got["vertices"]), bits(want["vertices"]))
    assert got["normals"].shape == want["normals"].shape and np.array_equal(bits(got["normals"]), bits(want["normals"]))
    if colors:
        assert got["colors"].shape == want["colors"].shape and np.array_equal(bits(got["colors"]), bits(want["colors"]))


def soup_of(g):
    return np.ascontiguousarray(g["soup"]).view(K.TRI_DTYPE).reshape(-1)


def weld_context(max_triangles):
    """a context for its triangle buffer alone (small volume, small camera)"""
    return K.Context(K.camera(*SMALL_CAM), 64, 3.0, levels=3, max_triangles=max_triangles)


def device_weld(ctx, color):
    ctx.weld_mesh(color, 1e-4)
    return ctx.read_mesh(color)


def count_cells(soup, thresh=1e-4):
    """distinct weld cells of a soup (meshData.h:750-753 in fp32)"""
    v = soup["v"]["pos"].reshape(-1, 3).astype(np.float32)
    r = np.float32(1.0 / float(np.float32(thresh)))
    c = (v * r + (np.sign(v) * 0.5).astype(np.float32)).astype(np.int32)
    return len(np.unique(c, axis=0))


# ---- 1. the reference's fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_device_weld_matches_reference_meshdata(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    col = bool(g["with_color"][0])
    soup = soup_of(g)
    ctx = weld_context(len(soup) + 16)
    ctx.write_triangles(soup)
    m = device_weld(ctx, col)
    same_mesh(m, g)
    nv, nf, rounds = ctx.mesh_counts()
    assert nv == len(g["vertices"]) and nf == len(g["faces"])
    assert 1 <= rounds <= count_cells(soup)
    if name == "mesh_stress":
        assert rounds >= 2                                        # clusters of adjacent cells: the selection really iterates
    assert np.array_equal(ctx.triangles().view(np.uint32), soup.view(np.uint32))          # the soup is only read
    ctx.close()


# ---- 2. a real soup at size ------------------------------------------------------------------------------------------------------------
def _bgr(cam, k):
    cols, rows = cam[0], cam[1]
    y, x = np.mgrid[0:rows, 0:cols]
    return np.stack([(x * 3 + k * 7) % 256, (y * 5 + x) % 256, (x + 2 * y + 31 * k) % 256], axis=-1).astype(np.uint8)


_SOUPS = {}


def scene_context(res, size, color, max_triangles):
    """Scene S fused from a few ground-truth poses and extracted: the context with its soup in the buffer.  The integration gate is
    the depth gate (4 m, not the stock 2 m), so that the box's back wall is fused too: 256^3 @ 3 m then gives more than 100 000 triangles"""
    cam = S.vga_camera()
    ctx = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3, max_triangles=max_triangles, has_color=color)
    trunc = max(P["integrate_sdf_trunc"], 5 * size / res)
    for k in (0, 4, 8, 12):
        pose = S.trajectory_pose(k, size).astype(np.float32)
        ctx.upload_depth_mm(S.render_depth_mm(pose, cam, size))
        if color:
            ctx.upload_rgb(_bgr(cam, k))
        ctx.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
        ctx.integrate(pose, trunc, P["depth_trunc_max"], has_color=color)
    ctx.marching_cubes(300 * size / res, has_color=color)
    return ctx


def scene_soup(res, size, color):
    key = (res, size, color)
    if key not in _SOUPS:
        ctx = scene_context(res, size, color, 3_000_000)
        _SOUPS[key] = ctx.triangles()
        ctx.close()
    return _SOUPS[key]


@pytest.mark.parametrize("res,size,color", [(256, 3.0, False), (256, 3.0, True), (512, 4.0, False)])
def test_device_weld_matches_host_weld_on_scene_soup(res, size, color):
    """Scene S, VGA, four frames fused at ground-truth poses, kf_marching_cubes, then kf_weld_mesh on the context that extracted
    against the host weld (the fixture-pinned yardstick) of the same read-back soup.  The 512^3 @ 4 m case is C2's volume.
    Measured on an MI355X box: 256^3 @ 3 m gives 116 679 triangles -> 61 277 vertices, 115 647 faces in 3 rounds (with and without
    colour); 512^3 @ 4 m gives 456 871 triangles -> 234 269 vertices, 452 884 faces in 3 rounds; the three cases together, host welds
    included, ran in under 4 s, far below the minute allowed for the 512^3 case's host side.  profiles/weld_c2.json has both sides'
    times on C2's own (2 m gate) soup."""
    ctx = scene_context(res, size, color, 3_000_000)
    soup = ctx.triangles()
    _SOUPS[(res, size, color)] = soup
    m = device_weld(ctx, color)
    nv, nf, rounds = ctx.mesh_counts()
    print("scene soup %d^3 color=%d: %d triangles -> %d vertices, %d faces, %d rounds" % (res, color, len(soup), nv, nf, rounds))
    host = H.mesh_from_soup(soup, color)
    assert len(soup) > 100000 and nv < len(soup) and nf < len(soup)       # not vacuous: a real weld, and at least one face dropped
    same_mesh(m, host)
    if color:
        assert len(np.unique(bits(m["colors"])[:, :3], axis=0)) > 100        # real colours went through
    assert np.array_equal(ctx.triangles().view(np.uint32), soup.view(np.uint32))
    ctx.close()


# ---- 3. determinism and reuse ------------------------------------------------------------------------------------------------------------
def test_same_soup_same_bytes_on_one_context_and_on_a_fresh_one():
    soup = scene_soup(256, 3.0, False)
    a = weld_context(len(soup))
    a.write_triangles(soup)
    m1 = device_weld(a, False)
    c1 = a.mesh_counts()
    m2 = device_weld(a, False)
    assert c1 == a.mesh_counts()
    b = weld_context(len(soup))
    b.write_triangles(soup)
    m3 = device_weld(b, False)
    assert c1 == b.mesh_counts()
    for k in ("vertices", "normals", "faces"):
        assert m1[k].tobytes() == m2[k].tobytes() == m3[k].tobytes(), k
    a.close(); b.close()


def test_small_soup_after_large_one_reuses_the_scratch():
    big = scene_soup(256, 3.0, False)
    ctx = weld_context(len(big))
    ctx.write_triangles(big)
    same_mesh(device_weld(ctx, False), H.mesh_from_soup(big, False))
    for name in ("mesh_stress", "mesh_s64_color"):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        ctx.write_triangles(soup_of(g))
        same_mesh(device_weld(ctx, bool(g["with_color"][0])), g)
    ctx.weld_release()                                            # and from nothing again
    ctx.write_triangles(big[:5000])
    same_mesh(device_weld(ctx, False), H.mesh_from_soup(big[:5000], False))
    ctx.close()


def test_appended_extraction_welds_to_the_single_soups_mesh():
    """kf_marching_cubes appends (the reference never clears its counter): called twice, every triangle is there twice, and every
    second copy is a duplicate face -- the mesh is the single soup's."""
    g = np.load(os.path.join(GOLD, "s64.npz"))
    ctx = K.Context(K.camera(*SMALL_CAM), 64, 3.0, levels=3, max_triangles=400000)
    ctx.upload_volume(g["tsdf"], g["weight"])
    thr = 300 * 3.0 / 64
    ctx.marching_cubes(thr)
    single = ctx.triangles()
    m1 = device_weld(ctx, False)
    ctx.marching_cubes(thr)
    twice = ctx.triangles()
    assert len(twice) == 2 * len(single) and np.array_equal(twice[len(single):].view(np.uint32), single.view(np.uint32))
    m2 = device_weld(ctx, False)
    same_mesh(m2, m1)
    same_mesh(m2, np.load(os.path.join(GOLD, "mesh_s64.npz")))
    ctx.close()


# ---- 4. through the classes --------------------------------------------------------------------------------------------------------------
def test_save_mesh_with_device_weld_matches_reference_meshdata_fixture(tmp_path):
    g = np.load(os.path.join(GOLD, "s64.npz"))
    m = np.load(os.path.join(GOLD, "mesh_s64.npz"))
    app = H.App(64, 3.0, SMALL_CAM, max_triangles=400000)
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*SMALL_CAM), 64, 3.0)
    ctx.upload_volume(g["tsdf"], g["weight"])
    app.set_device_weld(True)
    ntri = app.generate_mesh()
    assert ntri == len(m["soup"])
    with pytest.raises(K.KfError):
        ctx.mesh_counts()                                         # nothing has welded on the device yet
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        ok, nv, nf = app.save_mesh("mesh.obj")
        assert ok and nv == len(m["vertices"]) and nf == len(m["faces"])
        assert ctx.mesh_counts()[:2] == (nv, nf)                  # ... and now it has: saveMesh took the device path
        same_mesh(H.app_mesh(), m)
        assert np.array_equal(np.frombuffer(open("mesh.obj", "rb").read(), np.uint8), m["obj"])
        ok, nv, nf = app.save_mesh("mesh.ply")
        assert ok
        got = _ply_mask_alpha(np.frombuffer(open("mesh.ply", "rb").read(), np.uint8), nv, False)
        assert np.array_equal(got, _ply_mask_alpha(m["ply"], nv, False))
        app.set_device_weld(False)                                # and the host path still gives the same file
        ok, _, _ = app.save_mesh("mesh2.obj")
        assert ok and open("mesh2.obj", "rb").read().replace(b"mesh2.obj", b"mesh.obj") == open("mesh.obj", "rb").read()
    finally:
        os.chdir(cwd)
    app.close()


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------------
def test_edges():
    import ctypes as C
    g = np.load(os.path.join(GOLD, "mesh_s32.npz"))
    soup = soup_of(g)
    ctx = weld_context(len(soup))
    lib = ctx.lib
    assert lib.kf_read_mesh(ctx.h, None, None, None, None) == 1002             # before any weld
    assert lib.kf_mesh_counts(ctx.h, None, None, None) == 1002
    ctx.weld_mesh(False, 1e-4)                                                # empty buffer
    assert ctx.mesh_counts() == (0, 0, 0)
    m = ctx.read_mesh()
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3)
    ctx.write_triangles(soup)
    assert lib.kf_weld_mesh(ctx.h, 0, C.c_float(0.0)) == 1001
    assert lib.kf_weld_mesh(ctx.h, 0, C.c_float(-1.0)) == 1001
    assert lib.kf_write_triangles(ctx.h, soup.ctypes.data_as(C.c_void_p), 1, len(soup)) == 1001      # one past max_triangles
    same_mesh(device_weld(ctx, False), g)
    assert np.array_equal(ctx.triangles().view(np.uint32), soup.view(np.uint32))
    ctx.write_triangles(soup[:10], first=5)                                   # the count becomes first + count
    assert len(ctx.triangles()) == 15
    ctx.clear_triangles()
    ctx.weld_mesh(False, 1e-4)
    assert ctx.mesh_counts() == (0, 0, 0)
    ctx.close()
