"""Child process of test_gpu_raycast_forms.py: raycast every scenario of raycast_scenarios.py on the GPU and save what came out -- model vertices and
normals, RGB where colour is on, levels 1 and 2 of the two maps' pyramids, the form of every call (kf_get_raycast_form) -- to the .npz named on the
command line.  The raycast's environment switches (KF_RAYCAST_*) are read once per process: the parent starts one child per switch set.

    raycast_forms_child.py OUT.npz VOLUME_DIR

VOLUME_DIR holds the analytic volumes as <id>_tsdf.npy / <id>_weight.npy / <id>_rgb.npy, written by the parent.  The fused volume is fused here,
and its planes are saved too (the parent compares them with the oracle's before it compares a map).

Levels 1 and 2 are read straight after the raycast when the launch wrote them (kf_raycast_form::pyramid), after kf_downsample_model_* otherwise."""
import os
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite: initialised after the library's, it finds no device)

import raycast_scenarios as R          # noqa: E402
from hybkinectfu_amd import lib as K   # noqa: E402

P = R.P
FORM_FIELDS = [name for name, _ in K.RaycastForm._fields_]


def key(k):
    return k.replace("/", "__")


def run(vol, voldir, out):
    vid, res, size, color, cams = vol
    data = None
    for cam, _ in cams:
        ctx = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3, has_color=color)
        if vid == "fused":
            R.fuse_gpu(ctx)
            if "fused_tsdf" not in out:
                t, w = ctx.download_volume()
                out["fused_tsdf"], out["fused_weight"] = t.view(np.uint32), w.view(np.uint32)
        else:
            if data is None:
                data = [np.load(os.path.join(voldir, "%s_%s.npy" % (vid, p)), mmap_mode="r") for p in ("tsdf", "weight")]
                data.append(np.load(os.path.join(voldir, vid + "_rgb.npy")) if color else None)
            ctx.upload_volume(data[0], data[1], data[2])
        for call in R.calls(vol):
            k, ccam, _, pose, near, far = call
            if ccam != cam:
                continue
            ctx.raycast(pose, R.inc_for(res, size), near, far, has_color=color)
            f = ctx.raycast_form()
            out[key(k) + "_form"] = np.array([f[n] for n in FORM_FIELDS], np.int64)
            out[key(k) + "_v"] = ctx.download_map(K.MAP_MODEL_VERTICES).view(np.uint32)
            out[key(k) + "_n"] = ctx.download_map(K.MAP_MODEL_NORMALS).view(np.uint32)
            if color:
                out[key(k) + "_rgb"] = ctx.download_map(K.MAP_RAYCAST_RGB)
            if not f["pyramid"]:
                ctx.downsample(model=True)
            for lv in (1, 2):
                out[key(k) + "_v%d" % lv] = ctx.download_map(K.MAP_MODEL_VERTICES, lv).view(np.uint32)
                out[key(k) + "_n%d" % lv] = ctx.download_map(K.MAP_MODEL_NORMALS, lv).view(np.uint32)
        ctx.close()


def main(argv):
    path, voldir = argv[1], argv[2]
    out = {}
    for vol in R.VOLUMES:
        run(vol, voldir, out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv)
