"""GPU: the C++ host classes (HybKinectfu / CameraPoseFinderICP / CameraPoseFinderSDF / MeshGeneratorMarchingcube) run a
short sequence end to end; poses are compared with the CPU oracle running the same per-frame path."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = S.STOCK


def oracle_sequence(res, size, cam, trunc, n, sdf=False):
    ocam = O.Cam.make(*cam)
    vol = O.OVolume(res, size, P["volume_max_weight"])
    pose = S.pose0(size)
    poses, tracked = [], []
    mv = mn = None
    for k in range(n):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        tr = O.trunc_depth(O.depth_mm_to_m(mm), P["depth_trunc_min"], P["depth_trunc_max"])
        fl = O.bilateral(tr, P["filter_sigma_pixel"], P["filter_sigma_depth"])
        v = O.depth_to_vertices(fl, ocam)
        nn = O.vertices_to_normals(v)
        ok = True
        if k > 0:
            if sdf:
                ok, pose, _ = O.sdf_estimate(vol, tr, ocam, P["sdf_max_iter_nums"], P["camera_shake_dist"], P["camera_shake_angle"], pose)
            else:
                ok, pose = O.icp_estimate(O.pyramid(v, 3), O.pyramid(nn, 3, True), O.pyramid(mv, 3), O.pyramid(mn, 3, True), ocam,
                                          P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"], pose)
        if ok:
            O.integrate(vol, tr, nn, None, False, False, pose, trunc, 2.0, ocam, ocam)
        mv, mn, _ = O.raycast(vol, False, pose, 0.7 * trunc, ocam, P["depth_trunc_min"], P["depth_trunc_max"])
        poses.append(np.array(pose).copy()); tracked.append(ok)
    return poses, tracked, vol


@pytest.mark.parametrize("host_loop", [False, True])
def test_hybkinectfu_icp_sequence(host_loop, tmp_path):
    res, size, cam = 128, 3.0, S.vga_camera()
    trunc = 5 * size / res
    n = 5
    o_poses, o_tracked, ovol = oracle_sequence(res, size, cam, trunc, n)
    floor = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "floor_h128.npz"))
    meta = json.loads(str(floor["meta"]))
    assert meta["res"] == res and meta["size"] == size and abs(meta["kw"]["sdf_trunc"] - trunc) < 1e-9      # the fixture is this configuration
    assert np.array_equal(np.stack(o_poses).astype(np.float32).view(np.uint32), floor["poses"][:n].view(np.uint32))
    floor_t, floor_r = meta["floor_dt_m"], meta["floor_dr"]
    app = H.App(res, size, cam, host_loop=host_loop, sdf_trunc=trunc, max_triangles=600000)
    for k in range(n):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        ok = app.process_frame(mm, k)
        tracked, pose = app.pose()
        assert ok == o_tracked[k] == True
        gt = S.trajectory_pose(k, size)
        # End to end the two sides do not see identical tracker inputs (device __expf in the bilateral filter, another summation
        # order, a volume fused with last-bit-different poses).  How much that may move the pose is MEASURED: the oracle against
        # last-bit-perturbed copies of itself on exactly this configuration (tests/golden/floor_h128.npz, tests/tracking_floor.py;
        # a few micrometres) -- the host classes must stay within twice that floor (round 2 allowed 2e-3 here).
        assert np.max(np.abs(pose[:3, 3] - o_poses[k][:3, 3])) <= 2 * floor_t, (k, pose, o_poses[k])
        assert np.max(np.abs(pose[:3, :3] - o_poses[k][:3, :3])) <= 2 * floor_r
        assert np.max(np.abs(pose[:3, 3] - gt[:3, 3])) < 6e-3
    ntri = app.generate_mesh()
    otris = O.marching_cubes(ovol, False, 300 * size / res, 600000)
    assert abs(ntri - len(otris)) <= 0.05 * len(otris)          # the volumes differ only through the mm-level pose differences
    path = str(tmp_path / "hybkf_test_mesh.obj")
    ok, nv, nf = app.save_mesh(path)
    assert ok and os.path.getsize(path) > 1000 and nf <= ntri and nv < 3 * ntri // 2
    gm = H.app_mesh()["faces"]                                  # no degenerate, no duplicate face survives (meshData.cpp:281, :42-82)
    assert not np.any((gm[:, 0] == gm[:, 1]) | (gm[:, 0] == gm[:, 2]) | (gm[:, 1] == gm[:, 2]))
    txt = open(path).read().splitlines()
    assert sum(1 for l in txt if l.startswith("v ")) == nv and sum(1 for l in txt if l.startswith("f ")) == nf
    app.close()


def test_hybkinectfu_sdf_tracker_sequence():
    res, size, cam = 128, 3.0, S.vga_camera()
    trunc = 5 * size / res
    n = 4
    o_poses, o_tracked, _ = oracle_sequence(res, size, cam, trunc, n, sdf=True)
    floor = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "floor_sdf128.npz"))
    meta = json.loads(str(floor["meta"]))                     # oracle vs last-bit-perturbed oracle, this configuration and tracker
    assert meta["res"] == res and meta["kw"]["sdf_tracker"] and np.array_equal(np.stack(o_poses).astype(np.float32).view(np.uint32), floor["poses"][:n].view(np.uint32))
    app = H.App(res, size, cam, sdf_tracker=True, sdf_trunc=trunc)
    for k in range(n):
        ok = app.process_frame(S.render_depth_mm(S.trajectory_pose(k, size), cam, size), k)
        tracked, pose = app.pose()
        assert ok == o_tracked[k]
        if ok:
            assert np.max(np.abs(pose[:3, 3] - o_poses[k][:3, 3])) <= 2 * meta["floor_dt_m"], (k, pose, o_poses[k])
            assert np.max(np.abs(pose[:3, :3] - o_poses[k][:3, :3])) <= 2 * meta["floor_dr"]
    app.close()


def test_save_mesh_matches_reference_meshdata_fixture(tmp_path):
    """MeshGeneratorMarchingcube::generateMesh + saveMesh on the golden 64^3 volume: the GPU's triangle soup equals the soup the
    reference-MeshData fixture was made from (tests/golden/mesh_s64.npz, tools/make_mesh_golden.py), and the saved mesh --
    vertex array, face INDICES, normals, OBJ bytes -- equals what the reference's own ml::MeshData / ml::MeshIO produced."""
    from hybkinectfu_amd import lib as K
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "s64.npz"))
    m = np.load(os.path.join(gold, "mesh_s64.npz"))
    cam = (160, 120, 79.5, 59.5, 131.25, 131.25)
    app = H.App(64, 3.0, cam, max_triangles=400000)
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), 64, 3.0)
    ctx.upload_volume(g["tsdf"], g["weight"])
    ntri = app.generate_mesh()
    soup = ctx.triangles()
    assert ntri == len(soup) == len(m["soup"])
    assert np.array_equal(soup.view(np.uint32).reshape(-1, 18), m["soup"].view(np.uint32))            # same soup, same order
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        ok, nv, nf = app.save_mesh("mesh.obj")
        assert ok and nv == len(m["vertices"]) and nf == len(m["faces"])
        got = H.app_mesh()
        assert np.array_equal(got["faces"], m["faces"])
        assert np.array_equal(got["vertices"].view(np.uint32), m["vertices"].view(np.uint32))
        assert np.array_equal(got["normals"].view(np.uint32), m["normals"].view(np.uint32))
        assert np.array_equal(np.frombuffer(open("mesh.obj", "rb").read(), np.uint8), m["obj"])
    finally:
        os.chdir(cwd)
    app.close()
