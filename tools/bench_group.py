"""Slab groups on C4 (1024^3 @ 6 m, VGA, depth gates 6 m, device-resident frames): frames/s and merge time per frame of each leg, one JSON
line per leg.

    python tools/bench_group.py [--steps 60] [--warmup 10] [--legs whole,rccl1,local2,local4,local8,rcclall] [--color]

whole     one whole-volume context (kf_raycast_volume, no merge)
rccl1     KF_GROUP_RCCL_ALL at world 1 on device 0: the native merge with RCCL's collectives, nothing to exchange
localN    KF_GROUP_LOCAL, N equal slabs on device 0: every member marches every ray and tracks the whole image, so this leg is a protocol
          check, not a speed-up -- it is expected to run slower than `whole`
rcclall   KF_GROUP_RCCL_ALL over every visible device (skipped below two)

--color   the same legs with colour (the reference's stock switches use_color = 1, color_angle_weight = 1): a whole-volume colour context, colour groups,
          one random BGR image per frame resident beside the depth frames.  Each line then also names the bytes per pixel the SUM all-reduce
          carries (16 instead of 12) and the fusion kernel the members ran (colour excludes deferred weights: the plain kernel at 1024^3)

Frames/s: wall clock over `steps` frames enqueued back to back after `warmup` frames, one synchronisation at the end.  Merge: the group's
hipEvent pair around steps 6-9 of each timed frame (kf_group_merge_timing), on member 0's stream."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first)

from hybkinectfu_amd import group as G      # noqa: E402
from hybkinectfu_amd import lib as K        # noqa: E402
from hybkinectfu_amd import pipeline as PL  # noqa: E402
from hybkinectfu_amd import scene as S      # noqa: E402

P = S.STOCK
RES, SIZE, GATE = 1024, 6.0, 6.0
INC = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]


def frames_on(device, n_unique):
    cam = S.vga_camera()
    return [torch.from_numpy(S.render_depth_mm(S.trajectory_pose(k, SIZE), cam, SIZE).astype(np.int16)).to(torch.device("cuda", device))
            for k in range(n_unique)]


def rgb_on(device, n_unique):
    cam = S.vga_camera()
    rng = np.random.default_rng(1234)
    return [torch.from_numpy(rng.integers(0, 256, (cam[1], cam[0], 3)).astype(np.uint8)).to(torch.device("cuda", device)) for _ in range(n_unique)]


def fusion_kernel(ctx):
    f = ctx.fusion_form()
    return dict(fusion_kernel={1: "pairs", 2: "pairs_pipe", 3: "bricks"}.get(f["kernel"], "none"), fusion_defer=f["defer"], fusion_color=f["color"])


def run_whole(frames, warmup, steps, rgbs=None):
    kcam = K.camera(*S.vga_camera())
    ctx = K.Context(kcam, RES, SIZE, P["volume_max_weight"], levels=3, has_color=rgbs is not None)
    ctx.set_pose(S.pose0(SIZE))

    def one(k):
        ctx.set_depth_mm_device(frames[k % len(frames)].data_ptr())
        if rgbs is not None:
            ctx.set_rgb_device(rgbs[k % len(rgbs)].data_ptr())
        ctx.preprocess(P["depth_trunc_min"], GATE, P["filter_sigma_pixel"], P["filter_sigma_depth"])
        ctx.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
        ctx.integrate(None, P["integrate_sdf_trunc"], GATE, has_color=rgbs is not None, angle_weight=rgbs is not None)
        ctx.raycast(None, INC, P["depth_trunc_min"], GATE, has_color=rgbs is not None)
    for k in range(warmup):
        one(k)
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        one(k)
    ctx.sync()
    dt = time.perf_counter() - t0
    st = ctx.stats(observed=False)
    extra = fusion_kernel(ctx) if rgbs is not None else {}
    ctx.close()
    return dict(frames_per_s=steps / dt, merge_us_per_frame=None, frames_lost=int(st["frames_lost"]), **extra)


def run_group(g, frames_per_member, warmup, steps, rgb_per_member=None):
    def one(k):
        if rgb_per_member is not None:
            if len(frames_per_member) == 1:
                g.frame(frames_per_member[0][k % len(frames_per_member[0])].data_ptr(), k, rgb=rgb_per_member[0][k % len(rgb_per_member[0])].data_ptr())
            else:
                g.frame_members([f[k % len(f)].data_ptr() for f in frames_per_member], k, rgb_ptrs=[f[k % len(f)].data_ptr() for f in rgb_per_member])
        elif len(frames_per_member) == 1:
            g.frame(frames_per_member[0][k % len(frames_per_member[0])].data_ptr(), k)
        else:
            g.frame_members([f[k % len(f)].data_ptr() for f in frames_per_member], k)
    for k in range(warmup):
        one(k)
    g.sync()
    g.merge_timing(True)
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        one(k)
    g.sync()
    dt = time.perf_counter() - t0
    ms, n = g.merge_ms()
    g.track_result(check_lockstep=True)
    lost = int(g.members()[0].stats(observed=False)["frames_lost"])
    extra = {}
    if rgb_per_member is not None:
        npx = g.cam.cols * g.cam.rows
        extra = dict(sum_bytes_per_pixel=16, sum_bytes_per_frame=16 * npx, colourless_sum_bytes_per_frame=12 * npx, **fusion_kernel(g.members()[0]))
    g.close()
    return dict(frames_per_s=steps / dt, merge_us_per_frame=1e3 * ms / max(1, n), frames_lost=lost, **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--unique", type=int, default=20, help="distinct frames (on the device before the run)")
    ap.add_argument("--legs", default="whole,rccl1,local2,local4,local8,rcclall")
    ap.add_argument("--color", action="store_true", help="the legs with colour: colour contexts and groups, one BGR image per frame")
    args = ap.parse_args()
    kcam = K.camera(*S.vga_camera())
    params = G.stock_params(trunc_max=GATE, integ_dist=GATE)
    ndev = torch.cuda.device_count()
    box = dict(device=torch.cuda.get_device_name(0), visible_devices=ndev, rocm=torch.version.hip)
    frames0 = frames_on(0, args.unique)
    rgb0 = rgb_on(0, args.unique) if args.color else None
    ckw = dict(has_color=True, angle_weight=True) if args.color else {}
    for leg in args.legs.split(","):
        row = dict(config="C4", res=RES, size_m=SIZE, cam="640x480", warmup=args.warmup, steps=args.steps, leg=leg, color=bool(args.color), **box)
        if leg == "whole":
            row.update(members=1, backend="context", **run_whole(frames0, args.warmup, args.steps, rgb0))
        elif leg == "rccl1":
            g = G.Group.rccl_all(kcam, RES, SIZE, [0, RES], devices=[0], params=params, **ckw)
            row.update(members=1, backend="rccl_all", **run_group(g, [frames0], args.warmup, args.steps, [rgb0] if args.color else None))
        elif leg.startswith("local"):
            n = int(leg[5:])
            cuts = [0] + [r[1] for r in PL.slab_ranges(RES, n)]
            g = G.Group.local(kcam, RES, SIZE, cuts, params=params, **ckw)
            row.update(members=n, backend="local", halo=g.halo, **run_group(g, [frames0], args.warmup, args.steps, [rgb0] if args.color else None))
        elif leg == "rcclall":
            if ndev < 2:
                row.update(skipped="fewer than two visible devices")
            else:
                cuts = [0] + [r[1] for r in PL.slab_ranges(RES, ndev)]
                g = G.Group.rccl_all(kcam, RES, SIZE, cuts, devices=list(range(ndev)), params=params, **ckw)
                frames = [frames0] + [frames_on(d, args.unique) for d in range(1, ndev)]
                rgbs = [rgb0] + [rgb_on(d, args.unique) for d in range(1, ndev)] if args.color else None
                row.update(members=ndev, backend="rccl_all", halo=g.halo, **run_group(g, frames, args.warmup, args.steps, rgbs))
        else:
            raise SystemExit("unknown leg " + leg)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
