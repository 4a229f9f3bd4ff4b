"""Child process of test_gpu_group.py: a slab group over RCCL against a plain whole-volume lib.Context driven through the same calls, bit for
bit -- pose after every frame, model maps (levels 0-2) after every frame, and the volume (tsdf, weight) after the last one.  Exit status 0 and
"group rccl ok" on success; an assertion otherwise.  One process per RCCL leg, so a stuck collective ends one child and not the suite.

    group_rccl_child.py all1      RCCL_ALL at world 1 on device 0 (ncclCommInitAll)
    group_rccl_child.py rank1     RCCL_RANK at world 1 on device 0 (ncclCommInitRank with kf_group_unique_id)
    group_rccl_child.py alldev    RCCL_ALL over every visible device, one member per device, each reading the frame on its own device"""
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


def whole_frame(ctx, dev_mm, k, inc):
    ctx.set_depth_mm_device(dev_mm)
    ctx.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
    ctx.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
    ctx.integrate(None, P["integrate_sdf_trunc"], P["integrate_depth_trunc"])
    ctx.raycast(None, inc, P["depth_trunc_min"], P["depth_trunc_max"])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def main(mode):
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    inc = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]
    ndev = torch.cuda.device_count()
    if mode == "all1":
        g = G.Group.rccl_all(kcam, res, size, [0, res], devices=[0], max_triangles=600000)
    elif mode == "rank1":
        g = G.Group.rccl_rank(kcam, res, size, [0, res], device=0, uid=G.unique_id(), rank=0, world=1, max_triangles=600000)
    elif mode == "alldev":
        assert ndev >= 2, ndev
        cuts = [0] + [r[1] for r in PL.slab_ranges(res, ndev)]
        g = G.Group.rccl_all(kcam, res, size, cuts, devices=list(range(ndev)), max_triangles=600000)
    else:
        raise SystemExit("unknown mode " + mode)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, max_triangles=600000)
    whole.set_pose(S.pose0(size))
    devs = [0] if mode != "alldev" else list(range(ndev))
    g.merge_timing(True)
    for k in range(FRAMES):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        on = [torch.from_numpy(mm.astype(np.int16)).to(torch.device("cuda", d)) for d in devs]
        whole_frame(whole, on[0].data_ptr(), k, inc)
        if mode == "alldev":
            g.frame_members([t.data_ptr() for t in on], k)
        else:
            g.frame(on[0].data_ptr(), k)
        ok_g, pose_g, st_g, _ = g.track_result(check_lockstep=True)
        ok_w, pose_w, st_w, _ = whole.track_result()
        assert ok_g == ok_w and ok_w and st_g == st_w, (k, ok_g, ok_w, st_g, st_w)
        assert np.array_equal(bits(pose_g), bits(pose_w)), k
        for m in g.members():
            for level in range(3):
                for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                    assert np.array_equal(bits(m.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (k, level, map_id)
        g.sync()                                  # (the frames' tensors may go)
        torch.cuda.synchronize()
    tw, ww = whole.download_volume()
    assert int((ww > 0).sum()) > 100000
    for m in g.members():
        z0, z1 = m.owned
        t, w = m.download_volume(z0, z1)
        assert np.array_equal(bits(t), bits(tw[z0:z1])) and np.array_equal(w, ww[z0:z1]), (z0, z1)
    ms, n = g.merge_ms()
    assert n == FRAMES and ms > 0.0, (ms, n)
    g.close()
    whole.close()
    print("group rccl ok: %s, %d frames, %d members, merge %.1f us per frame" % (mode, FRAMES, len(devs), 1e3 * ms / n))


if __name__ == "__main__":
    main(sys.argv[1])
