"""Child process of test_gpu_slab_color.py: a COLOUR slab group over RCCL against a plain whole-volume colour lib.Context driven through the same
calls, bit for bit -- pose, model maps (levels 0-2) and the RGB map after every frame, the volume (tsdf, weight, colour bytes) after the last one.
Exit status 0 and "group colour rccl ok" on success.  One process per RCCL leg, so a stuck collective ends one child and not the suite.

    group_color_rccl_child.py all1      RCCL_ALL at world 1 on device 0
    group_color_rccl_child.py rank1     RCCL_RANK at world 1 on device 0
    group_color_rccl_child.py alldev    RCCL_ALL over every visible device, one member per device, each reading the frames on its own device"""
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite)

from hybkinectfu_amd import group as G      # noqa: E402
from hybkinectfu_amd import lib as K        # noqa: E402
from hybkinectfu_amd import pipeline as PL  # noqa: E402
from hybkinectfu_amd import scene as S      # noqa: E402

P = S.STOCK
FRAMES = 6
GATE = 4.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def main(mode):
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    inc = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]
    params = G.stock_params(trunc_max=GATE, integ_dist=GATE)
    ndev = torch.cuda.device_count()
    kw = dict(max_triangles=600000, params=params, has_color=True, angle_weight=True)
    if mode == "all1":
        g = G.Group.rccl_all(kcam, res, size, [0, res], devices=[0], **kw)
    elif mode == "rank1":
        g = G.Group.rccl_rank(kcam, res, size, [0, res], device=0, uid=G.unique_id(), rank=0, world=1, **kw)
    elif mode == "alldev":
        assert ndev >= 2, ndev
        cuts = [0] + [r[1] for r in PL.slab_ranges(res, ndev)]
        g = G.Group.rccl_all(kcam, res, size, cuts, devices=list(range(ndev)), **kw)
    else:
        raise SystemExit("unknown mode " + mode)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, max_triangles=600000, has_color=True)
    whole.set_pose(S.pose0(size))
    devs = [0] if mode != "alldev" else list(range(ndev))
    rng = np.random.default_rng(17)
    for k in range(FRAMES):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        rgb = rng.integers(0, 256, (cam[1], cam[0], 3)).astype(np.uint8)
        on = [torch.from_numpy(mm.astype(np.int16)).to(torch.device("cuda", d)) for d in devs]
        on_rgb = [torch.from_numpy(rgb).to(torch.device("cuda", d)) for d in devs]
        whole.set_depth_mm_device(on[0].data_ptr())
        whole.set_rgb_device(on_rgb[0].data_ptr())
        whole.preprocess(P["depth_trunc_min"], GATE, P["filter_sigma_pixel"], P["filter_sigma_depth"])
        whole.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
        whole.integrate(None, P["integrate_sdf_trunc"], GATE, has_color=True, angle_weight=True)
        whole.raycast(None, inc, P["depth_trunc_min"], GATE, has_color=True)
        if mode == "alldev":
            g.frame_members([t.data_ptr() for t in on], k, rgb_ptrs=[t.data_ptr() for t in on_rgb])
        else:
            g.frame(on[0].data_ptr(), k, rgb=on_rgb[0].data_ptr())
        ok_g, pose_g, st_g, _ = g.track_result(check_lockstep=True)
        ok_w, pose_w, st_w, _ = whole.track_result()
        assert ok_g == ok_w and ok_w and st_g == st_w, (k, ok_g, ok_w, st_g, st_w)
        assert np.array_equal(bits(pose_g), bits(pose_w)), k
        wrgb = whole.download_map(K.MAP_RAYCAST_RGB)
        assert int(wrgb.any(axis=-1).sum()) > 10000
        for m in g.members():
            for level in range(3):
                for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                    assert np.array_equal(bits(m.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (k, level, map_id)
            assert np.array_equal(m.download_map(K.MAP_RAYCAST_RGB), wrgb), k
        g.sync()                                  # (the frames' tensors may go)
        torch.cuda.synchronize()
    tw, ww, cw = whole.download_volume(color=True)
    assert int((ww > 0).sum()) > 100000 and int(np.count_nonzero(cw[ww > 0])) > 10000
    for m in g.members():
        z0, z1 = m.owned
        t, w, c = m.download_volume(z0, z1, color=True)
        assert np.array_equal(bits(t), bits(tw[z0:z1])) and np.array_equal(w, ww[z0:z1]) and np.array_equal(c, cw[z0:z1]), (z0, z1)
    thr = 300 * size / res
    whole.marching_cubes(thr, has_color=True)
    g.marching_cubes(thr)
    wt = whole.triangles()
    assert len(wt) > 1000 and g.triangles().tobytes() == wt.tobytes()
    g.close()
    whole.close()
    print("group colour rccl ok: %s, %d frames, %d members" % (mode, FRAMES, len(devs)))


if __name__ == "__main__":
    main(sys.argv[1])
