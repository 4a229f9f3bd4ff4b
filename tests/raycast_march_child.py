"""Child process of test_gpu_raycast_march.py: cast the cases named on the command line on the GPU and save the maps -- model vertices and normals,
levels 1 and 2 of their pyramids, the form of every call -- to an .npz.  The raycast's switches (KF_RAYCAST_*) are read once per process: the parent
starts one child per switch set.

    raycast_march_child.py OUT.npz VOLUME_DIR CASE [CASE ...]

CASE is an id of raycast_march_cases.CASES (a whole volume: every view of it), or `slabs` (the 128^3 volume once whole and once as two z-slabs whose
candidates are merged here the way test_gpu_slabs.py merges them).  VOLUME_DIR holds <volume id>_tsdf.npy / _weight.npy, written by the parent."""
import os
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite)

import raycast_march_cases as M        # noqa: E402
import raycast_scenarios as R          # noqa: E402
from hybkinectfu_amd import lib as K   # noqa: E402

P = R.P
FORM_FIELDS = [name for name, _ in K.RaycastForm._fields_]


def load(voldir, vid):
    return [np.load(os.path.join(voldir, "%s_%s.npy" % (vid, p)), mmap_mode="r") for p in ("tsdf", "weight")]


def save_maps(ctx, out, k):
    f = ctx.raycast_form()
    out[k + "_form"] = np.array([f[n] for n in FORM_FIELDS], np.int64)
    out[k + "_v"] = ctx.download_map(K.MAP_MODEL_VERTICES).view(np.uint32)
    out[k + "_n"] = ctx.download_map(K.MAP_MODEL_NORMALS).view(np.uint32)
    if not f["pyramid"]:
        ctx.downsample(model=True)
    for lv in (1, 2):
        out[k + "_v%d" % lv] = ctx.download_map(K.MAP_MODEL_VERTICES, lv).view(np.uint32)
        out[k + "_n%d" % lv] = ctx.download_map(K.MAP_MODEL_NORMALS, lv).view(np.uint32)


def run_whole(case, voldir, out):
    vid, res, size, cam, _ = case
    data = load(voldir, vid)
    ctx = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3)
    ctx.upload_volume(data[0], data[1], None)
    for k, name, pose, near, far in M.calls(case):
        ctx.raycast(pose, R.inc_for(res, size), near, far)
        save_maps(ctx, out, M.key(k))
    ctx.close()


def run_slabs(voldir, out):
    """two z-slabs of the 128^3 volume (the second one's stored layers start above layer 0), merged as the collective merges them: MIN over the
    crossings' parameters, the winner's candidate bits"""
    vid, res, size, cam, _ = M.SLAB_CASE
    data = load(voldir, vid)
    inc = R.inc_for(res, size)
    dev = torch.device("cuda", 0)
    slabs = [K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3, slab=r, halo=M.SLAB_HALO) for r in M.SLAB_RANGES]
    for c in slabs:
        z0, z1 = c.stored
        c.upload_volume(data[0][z0:z1], data[1][z0:z1], None)
    out["slabs_stored"] = np.array([c.stored for c in slabs], np.int64)
    for k, name, pose, near, far in M.calls(M.SLAB_CASE):
        cand = []
        for c in slabs:
            t = torch.empty((cam[1], cam[0]), dtype=torch.float32, device=dev)
            v = torch.empty((cam[1], cam[0], 4), dtype=torch.float32, device=dev)
            n = torch.empty((cam[1], cam[0], 4), dtype=torch.float32, device=dev)
            c.raycast_slab(pose, inc, near, far, t.data_ptr(), v.data_ptr(), n.data_ptr())
            c.sync()
            cand.append((t.cpu().numpy(), v.cpu().numpy().view(np.uint32), n.cpu().numpy().view(np.uint32)))
        tmin = np.minimum(cand[0][0], cand[1][0])
        mv, mn = np.zeros((cam[1], cam[0], 4), np.uint32), np.zeros((cam[1], cam[0], 4), np.uint32)
        owners = np.zeros((cam[1], cam[0]), np.int32)
        for t, v, n in cand:
            win = (t == tmin) & np.isfinite(t)
            mv += v * win[..., None].astype(np.uint32)
            mn += n * win[..., None].astype(np.uint32)
            owners += win
        out["slabs_" + M.key(k) + "_v"], out["slabs_" + M.key(k) + "_n"], out["slabs_" + M.key(k) + "_owners"] = mv, mn, owners
    for c in slabs:
        c.close()


def main(argv):
    path, voldir = argv[1], argv[2]
    out = {}
    for cid in argv[3:]:
        if cid == "slabs":
            run_slabs(voldir, out)
            run_whole(M.SLAB_CASE, voldir, out)
        else:
            run_whole(M.CASES[cid], voldir, out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv)
