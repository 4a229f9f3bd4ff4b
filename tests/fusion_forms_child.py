"""Child process of test_gpu_fusion_forms.py: fuse the scenarios of fusion_scenarios.py on the GPU and save what came out -- tsdf / weight bit planes,
colour bytes, per-frame update counts, observed-voxel counts where asked, the fusion form (kf_get_fusion_form) of every frame -- to the .npz named on
the command line.  The fusion pass's environment switches (KF_INTEGRATE_*, KF_CULL_*, KF_OBSERVED_COUNT) are read once per process: the parent
starts one child per switch set.

    fusion_forms_child.py OUT.npz [--ask ends|every] [--no-set-defer]

--ask: when kf_get_volume_stats (the observed-voxel count) is asked -- after the first and the last frame of a scenario, or after every frame (which
switches the fusion launches to their COUNT forms).  Update counts come from kf_get_fusion_counters, which asks nothing.
--no-set-defer: never call kf_set_defer (the environment and the volume's size decide on deferral)."""
import sys

import numpy as np
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite: initialised after the library's, it finds no device)

import fusion_scenarios as F           # noqa: E402
from hybkinectfu_amd import lib as K   # noqa: E402

P = F.P
FORM_FIELDS = [name for name, _ in K.FusionForm._fields_]


def run(name, sc, ask_every, set_defer, out):
    rcam = K.camera(*sc["rcam"]) if "rcam" in sc else None
    ctx = K.Context(K.camera(*sc["cam"]), sc["res"], sc["size"], sc["maxw"], levels=3, has_color=sc.get("has_color", False), rgb_cam=rcam,
                    slab=sc.get("slab"), halo=sc.get("halo", 0))
    assert ctx.stored == F.stored_range(sc), (ctx.stored, F.stored_range(sc))
    n = len(sc["frames"])
    upd, gt0, layers = np.zeros(n, np.uint64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    forms, poses, track_forms = np.zeros((n, len(FORM_FIELDS)), np.int64), np.zeros((n, 4, 4), np.float32), np.zeros(n, np.int64)
    tracked = sc.get("tracked", False)
    if tracked:
        ctx.set_pose(F.S.trajectory_pose(sc["frames"][0]["k"], sc["size"]).astype(np.float32))
    for i, fr in enumerate(sc["frames"]):
        pose, mm, rgb, tr, nrm = F.frame_inputs(name, sc, i)
        if set_defer and fr["defer"] is not None:
            ctx.set_defer(fr["defer"])                  # (before the preprocess: it builds the tile minima the deferred cull reads)
        ctx.upload_depth_mm(mm)
        ctx.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
        if fr["color"]:
            ctx.upload_rgb(rgb)
            ctx.upload_map(K.MAP_NEW_NORMALS, 0, nrm)
        if fr["layers"]:
            ctx.count_layer_work(1)
        if tracked:
            ctx.icp_track(i, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
            ok, pose, _, _ = ctx.track_result()
            assert ok, (name, i)
            track_forms[i] = ctx.last_form
            ctx.integrate(None, fr["trunc"], fr["dist"])
            ctx.raycast(None, 0.7 * fr["trunc"], P["depth_trunc_min"], P["depth_trunc_max"])
        else:
            ctx.integrate(pose, fr["trunc"], fr["dist"], has_color=fr["color"], angle_weight=fr["angled"])
        poses[i] = pose
        f = ctx.fusion_form()
        forms[i] = [f[k] for k in FORM_FIELDS]
        upd[i] = ctx.stats(observed=False)["updated_last"]
        if fr["layers"]:
            layers[i] = int(ctx.read_layer_work().sum())
        if ask_every or i in (0, n - 1):
            gt0[i] = ctx.stats()["weight_gt0"]          # (KF_STATS_CROSSCHECK=1: also checked against a sweep of the volume)
    t, w, c = ctx.download_volume(color=True) if sc.get("has_color") else ctx.download_volume() + (None,)
    out[name + "_tsdf"], out[name + "_weight"] = t.view(np.uint32), w.view(np.uint32)
    if c is not None:
        out[name + "_color"] = c
    out[name + "_upd"], out[name + "_gt0"], out[name + "_layers"], out[name + "_form"] = upd, gt0, layers, forms
    out[name + "_pose"], out[name + "_track_form"] = poses, track_forms
    out[name + "_tail"] = np.array(ctx.cull_tail_counts(), np.int64)
    ctx.close()                                         # (one live context at a time: a second one switches the persistent tracking loop off)


def main(argv):
    path = argv[1]
    ask_every = "--ask" in argv and argv[argv.index("--ask") + 1] == "every"
    set_defer = "--no-set-defer" not in argv
    out = {}
    for name in F.ORDER:
        run(name, F.SCENARIOS[name], ask_every, set_defer, out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv)
