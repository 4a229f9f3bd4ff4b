"""Child process of test_gpu_view_at.py: six frames of Scene S fused at 64 voxels with a brick store, the window shifted by (32, 0, 0), then
kf_render_view_at of the frame (0, 0, 0) -- the old place, half of it held by the store alone -- with the context camera and the device-resident pose;
prints one SHA-1 of the picture and of each float4 map.  The KF_RAYCAST_* switches are read once per process -- hence a process per setting."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_shift as G  # noqa: E402
from hybkinectfu_amd import lib as K  # noqa: E402

P = G.P


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).view(np.uint8)).hexdigest()


def main():
    ctx = G.make_ctx(64)
    ctx.brick_store_reserve(1024)
    G.fuse(ctx, range(6))
    ctx.shift_volume(32, 0, 0)
    cam = G.CAM
    dv = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device="cuda:0")
    dn = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device="cuda:0")
    ctx.render_view_at(K.VIEW_SHADED, (0, 0, 0), None, K.camera(*cam), 0.7 * 5 * ctx.size / ctx.res, P["depth_trunc_min"], P["depth_trunc_max"],
                       dv.data_ptr(), dn.data_ptr())
    img = ctx.read_view()
    out = dict(img=sha(img), v=sha(dv.cpu().numpy()), n=sha(dn.cpu().numpy()), hits=int((img[..., 3] == 255).sum()))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
