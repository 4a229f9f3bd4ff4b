"""Child process of test_gpu_group_view.py: merged views of a slab group over RCCL against the LOCAL group's, byte for byte, on the analytic
volume a104 of raycast_scenarios.py.  Exit status 0 and "group view rccl ok" on success; an assertion otherwise.  One process per RCCL leg, so
a stuck collective ends one child and not the suite.

    group_view_rccl_child.py all1      RCCL_ALL at world 1 on device 0
    group_view_rccl_child.py rank1     RCCL_RANK at world 1 on device 0 (the collective call of its one rank)
    group_view_rccl_child.py alldev    RCCL_ALL over every visible device, one member per device"""
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite)

import raycast_scenarios as R               # noqa: E402
from hybkinectfu_amd import group as G      # noqa: E402
from hybkinectfu_amd import lib as K        # noqa: E402
from hybkinectfu_amd import pipeline as PL  # noqa: E402

VIEWS = ("front+z", "back-z", "corner-mixed")


def fill(g, data):
    for m in g.members():
        s0, s1 = m.stored
        m.upload_volume(data[0][s0:s1], data[1][s0:s1])


def main(mode):
    vol = next(v for v in R.VOLUMES if v[0] == "a104")
    _, res, size, _, _ = vol
    data = R.volume_data(vol)
    kcam = K.camera(*R.ODD)
    params = G.stock_params()
    params.raycast = K.RaycastParams(R.inc_for(res, size))
    ndev = torch.cuda.device_count()
    if mode == "all1":
        g = G.Group.rccl_all(kcam, res, size, [0, res], devices=[0], params=params)
    elif mode == "rank1":
        g = G.Group.rccl_rank(kcam, res, size, [0, res], device=0, uid=G.unique_id(), rank=0, world=1, params=params)
    elif mode == "alldev":
        assert ndev >= 2, ndev
        n = min(ndev, res // 8)
        g = G.Group.rccl_all(kcam, res, size, [0] + [r[1] for r in PL.slab_ranges(res, n)], devices=list(range(n)), params=params)
    else:
        raise SystemExit("unknown mode " + mode)
    local = G.Group.local(kcam, res, size, [0, 56, 104], params=params)
    fill(g, data)
    fill(local, data)
    hits = 0
    for key, cam, view, pose, near, far in [c for c in R.calls(vol) if c[1] == R.RAGGED and c[2] in VIEWS]:
        for m in (K.VIEW_NORMALS, K.VIEW_SHADED):
            g.render_view(m, pose, K.camera(*cam), near, far)
            local.render_view(m, pose, K.camera(*cam), near, far)
            a, b = g.read_view(), local.read_view()
            assert a.shape == (cam[1], cam[0], 4) and np.array_equal(a, b), (key, m)
            assert int((a[..., 3] == 255).sum()) >= R.min_hits(view, cam), key
            hits += int((a[..., 3] == 255).sum())
    g.close()
    local.close()
    print("group view rccl ok: %s, %d views, %d hits" % (mode, 2 * len(VIEWS), hits))


if __name__ == "__main__":
    main(sys.argv[1])
