"""Child process of test_gpu_group_shift.py: a slab group over RCCL shifts its window (kf_group_shift_volume) and is compared, bit for bit, with a
plain whole-volume lib.Context doing kf_shift_volume in the same process: every member's stored layers, pose and origin after the shift, the model
maps after the merged raycast, and the frame that follows.  Exit status 0 and "group shift rccl ok" on success; an assertion otherwise.  One process
per RCCL leg, so a stuck exchange ends one child and not the suite.

    group_shift_rccl_child.py all1      RCCL_ALL at world 1 on device 0: the plan is empty
    group_shift_rccl_child.py rank1     RCCL_RANK at world 1 on device 0: the plan is empty, nothing is gathered
    group_shift_rccl_child.py alldev    RCCL_ALL over every visible device: one z shift that crosses every boundary (ncclSend / ncclRecv)"""
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite)

from hybkinectfu_amd import group as G      # noqa: E402
from hybkinectfu_amd import lib as K        # noqa: E402
from hybkinectfu_amd import pipeline as PL  # noqa: E402
from hybkinectfu_amd import scene as S      # noqa: E402

from group_rccl_child import bits, whole_frame  # noqa: E402

P = S.STOCK
FRAMES = 3


def main(mode):
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    inc = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]
    ndev = torch.cuda.device_count()
    if mode == "all1":
        cuts = [0, res]
        g = G.Group.rccl_all(kcam, res, size, cuts, devices=[0])
    elif mode == "rank1":
        cuts = [0, res]
        g = G.Group.rccl_rank(kcam, res, size, cuts, device=0, uid=G.unique_id(), rank=0, world=1)
    elif mode == "alldev":
        assert ndev >= 2, ndev
        cuts = [0] + [r[1] for r in PL.slab_ranges(res, ndev)]
        g = G.Group.rccl_all(kcam, res, size, cuts, devices=list(range(ndev)))
    else:
        raise SystemExit("unknown mode " + mode)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3)
    whole.set_pose(S.pose0(size))
    devs = [0] if mode != "alldev" else list(range(ndev))

    def one_frame(k):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        on = [torch.from_numpy(mm.astype(np.int16)).to(torch.device("cuda", d)) for d in devs]
        whole_frame(whole, on[0].data_ptr(), k, inc)
        if mode == "alldev":
            g.frame_members([t.data_ptr() for t in on], k)
        else:
            g.frame(on[0].data_ptr(), k)
        ok_g, pose_g, _, _ = g.track_result(check_lockstep=True)
        ok_w, pose_w, _, _ = whole.track_result()
        assert ok_g and ok_w and np.array_equal(bits(pose_g), bits(pose_w)), k
        g.sync()                                  # (the frames' tensors may go)
        torch.cuda.synchronize()

    def same_volume(what):
        tw, ww = whole.download_volume()
        for i, m in enumerate(g.members()):
            z0, z1 = m.stored
            t, w = m.download_volume(z0, z1)
            assert np.array_equal(bits(t), bits(tw[z0:z1])) and np.array_equal(bits(w), bits(ww[z0:z1])), (what, i)
        return ww

    for k in range(FRAMES):
        one_frame(k)
    assert int((same_volume("before") > 0).sum()) > 100000
    # every boundary is crossed: a shift of one brick layer feeds every member but the last from its upper neighbour
    d = (0, 0, 8)
    plan = G.shift_plan(res, cuts, g.halo, d[2])
    assert len(plan) == len(cuts) - 2, plan
    g.shift_volume(*d)
    whole.shift_volume(*d)
    same_volume("shifted")
    assert g.volume_origin() == whole.volume_origin() == d
    for m in g.members():
        assert np.array_equal(bits(m.track_result()[1]), bits(whole.track_result()[1]))
    g.raycast()
    whole.raycast(None, inc, P["depth_trunc_min"], P["depth_trunc_max"])
    whole.downsample(True)
    for m in g.members():
        for level in range(3):
            for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                assert np.array_equal(bits(m.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (level, map_id)
    # back across the boundaries the other way, two layers wide, and a refusal in between
    try:
        g.shift_volume(0, 0, 4)
        raise AssertionError("a shift by half a brick was accepted")
    except G.GroupError as e:
        assert e.status == G.ERR_ARG
    g.shift_volume(8, 0, -16)
    whole.shift_volume(8, 0, -16)
    same_volume("back")
    g.raycast()
    whole.raycast(None, inc, P["depth_trunc_min"], P["depth_trunc_max"])
    one_frame(FRAMES)
    same_volume("after the next frame")
    g.close()
    whole.close()
    print("group shift rccl ok: %s, %d members, %d transfers" % (mode, len(devs), len(plan)))


if __name__ == "__main__":
    main(sys.argv[1])
