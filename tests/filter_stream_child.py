"""The streamed sequence of test_gpu_filter_forms.py with no far gate (trunc_max = +inf), in one of its modes; run in-process by the test and, for
KF_PREFETCH_FUSED=0 (read once per process), as a child that saves the result to the .npz named on the command line.

    filter_stream_child.py OUT.npz MODE"""
import sys

import numpy as np
import torch

from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

P = S.STOCK
RES, SIZE, CAM, N = 384, 3.0, S.vga_camera(), 6            # the sequence of test_gpu_parity.test_prefetched_preprocess_is_bit_identical
MAPS = (K.MAP_RAW_DEPTH, K.MAP_TRUNCED_DEPTH, K.MAP_FILTERED_DEPTH, K.MAP_NEW_VERTICES, K.MAP_NEW_NORMALS, K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS)


def frames():
    return np.stack([S.render_depth_mm(S.trajectory_pose(k, SIZE), CAM, SIZE) for k in range(N)])


def run(mode):
    """mode: plain / prefetch (the filter rides in the ICP loop, the raycast takes the `behind` riders) / prefetch-per-step (a second live context
    forces one launch per Gauss-Newton step: the filter rides in the raycast).  Returns poses, maps, volume, each frame's tracking launch form and
    each frame's raycast form (kf_get_raycast_form fields kernel, fast)."""
    from hybkinectfu_amd.pipeline import SingleGpuPipeline
    wl = dict(trunc_max=float("inf"), integ_dist=P["integrate_depth_trunc"])
    dev = torch.from_numpy(frames().astype(np.int16)).cuda()
    fb = CAM[0] * CAM[1] * 2
    other = K.Context(K.camera(64, 48, 31.5, 23.5, 52.5, 52.5), 32, 3.0, levels=3) if mode == "prefetch-per-step" else None
    pipe = SingleGpuPipeline(K.camera(*CAM), RES, SIZE, wl)
    poses, track_forms, rc_forms = [], [], []
    for k in range(N):
        nxt = dev.data_ptr() + (k + 1) * fb if mode.startswith("prefetch") and k + 1 < N else None
        pipe.process_frame_device(dev.data_ptr() + k * fb, k, nxt)
        ok, pose, _, _ = pipe.track_result()
        assert ok, (mode, k)
        poses.append(pose.copy())
        track_forms.append(pipe.ctx.last_form)
        f = pipe.ctx.raycast_form()
        rc_forms.append((f["kernel"], f["fast"]))
    pipe.sync()
    if other is not None:
        other.close()
    maps = [pipe.ctx.download_map(m) for m in MAPS]
    t, w = pipe.ctx.download_volume()
    pipe.close()
    return dict(poses=np.stack(poses), maps=maps, tsdf=t, weight=w, track_forms=np.array(track_forms), rc_forms=np.array(rc_forms))


if __name__ == "__main__":
    torch.zeros(1, device="cuda:0")      # (torch's HIP runtime first, as everywhere in the suite)
    r = run(sys.argv[2])
    np.savez(sys.argv[1], poses=r["poses"], tsdf=r["tsdf"], weight=r["weight"], track_forms=r["track_forms"], rc_forms=r["rc_forms"],
             **{"map%d" % i: m for i, m in enumerate(r["maps"])})
