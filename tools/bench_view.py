#!/usr/bin/env python3
"""Viewer frames on C2 (512^3 @ 4 m, VGA, Scene S): one JSON line per leg.
  usage: tools/bench_view.py [device|stream|readback|all] [reps]
         tools/bench_view.py --group N [reps]
  --group N  merged views over a LOCAL slab group of N members at C2's volume (kf_group_render_view), two legs: the device time of a VGA merged view
            per mode next to kf_render_view on a whole-volume context fed the same frames, in the same run; and the group's stream rate with no view
            and with a VGA view after every frame, three alternating runs each
  device    kf_render_view per mode at 640x480, 1280x960 and 1920x1080 and kf_view_model_maps at VGA on C2's fused volume, each between a hipEvent
            pair on the context's stream (median of `reps`), next to the plain raycast kernel's own time for the same pose at VGA (stage 7)
  stream    frames/s of the device-frame pipeline with no view, a VGA view after every frame and one every fourth frame: three alternating runs each
  readback  kf_read_view of a VGA view (1.2 MB) against the two kf_download_map calls plus the numpy conversion it replaces"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from hybkinectfu_amd import group as G, lib as K, pipeline as PL, scene as S
import bench

group_n = 0
if len(sys.argv) > 1 and sys.argv[1] == "--group":
    group_n = int(sys.argv[2])
    del sys.argv[1:3]
    sys.argv.insert(1, "group")
leg = sys.argv[1] if len(sys.argv) > 1 else "all"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 21
wl = bench.workload(1, "c2")
cam, P, res, size = wl["cam"], S.STOCK, wl["res"], wl["size"]
med = statistics.median
NAMES = {K.VIEW_NORMALS: "normals", K.VIEW_SHADED: "shaded", K.VIEW_COLOR: "color"}
gpu = torch.cuda.get_device_name(0)


def fused_pipe(n_frames, color=False):
    frames, _ = S.make_stream(n_frames, cam, size)
    dev = torch.from_numpy(frames.astype(np.int16)).cuda()
    pipe = PL.SingleGpuPipeline(K.camera(*cam), res, size, dict(trunc_max=wl["trunc_max"], integ_dist=wl["integ_dist"], color=color))
    return pipe, dev, cam[0] * cam[1] * 2


def event_ms(ctx, fn, n):
    stream = torch.cuda.ExternalStream(ctx.stream)
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def leg_device():
    pipe, dev, fb = fused_pipe(12)
    ctx = pipe.ctx
    for k in range(12):
        pipe.process_frame_device(dev.data_ptr() + k * fb, k, None)
    ok, pose, _, _ = pipe.track_result()
    near, far = P["depth_trunc_min"], wl["trunc_max"]
    # the plain raycast kernel for the same pose at VGA: its own dispatch's time (stage 7)
    ctx.stage_timers(1 << 7)
    for _ in range(reps):
        ctx.raycast(pose, pipe.inc, near, far)
    ms, cnt = ctx.read_stage_ms()
    ctx.stage_timers(0)
    print(json.dumps(dict(tool="bench_view", leg="device", what="kf_raycast_volume kernel (stage 7)", cols=cam[0], rows=cam[1], device=gpu,
                          kernel_us=round(1e3 * float(ms[7]) / max(int(cnt[7]), 1), 2), reps=int(cnt[7]))))
    for scale, (c, r) in (("640x480", (640, 480)), ("1280x960", (1280, 960)), ("1920x1080", (1920, 1080))):
        f = 525.0 * c / 640.0
        vc = K.camera(c, r, (c - 1) / 2.0, (r - 1) / 2.0, f, f)
        for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
            fn = lambda: ctx.render_view(mode, pose, vc, pipe.inc, near, far)
            event_ms(ctx, fn, 3)
            t = event_ms(ctx, fn, reps)
            print(json.dumps(dict(tool="bench_view", leg="device", what="kf_render_view", mode=NAMES[mode], cols=c, rows=r, device=gpu,
                                  event_us_median=round(1e3 * med(t), 2), event_us_min=round(1e3 * min(t), 2), reps=reps)))
    for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
        fn = lambda: ctx.view_model_maps(mode)
        event_ms(ctx, fn, 3)
        t = event_ms(ctx, fn, reps)
        print(json.dumps(dict(tool="bench_view", leg="device", what="kf_view_model_maps", mode=NAMES[mode], cols=cam[0], rows=cam[1], device=gpu,
                              event_us_median=round(1e3 * med(t), 2), event_us_min=round(1e3 * min(t), 2), reps=reps)))
    pipe.close()
    # colour: a colour context of the same volume
    pipe, dev, fb = fused_pipe(6, color=True)
    ctx = pipe.ctx
    bgr = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (cam[1], cam[0], 3), dtype=np.uint8)).cuda()
    for k in range(6):
        ctx.set_rgb_device(bgr.data_ptr())
        pipe.process_frame_device(dev.data_ptr() + k * fb, k, None)
    ok, pose, _, _ = pipe.track_result()
    vc = K.camera(*cam)
    fn = lambda: ctx.render_view(K.VIEW_COLOR, pose, vc, pipe.inc, near, far)
    event_ms(ctx, fn, 3)
    t = event_ms(ctx, fn, reps)
    print(json.dumps(dict(tool="bench_view", leg="device", what="kf_render_view", mode="color", cols=cam[0], rows=cam[1], device=gpu,
                          event_us_median=round(1e3 * med(t), 2), event_us_min=round(1e3 * min(t), 2), reps=reps)))
    pipe.close()


def leg_stream(n=200, warm=20):
    frames, _ = S.make_stream(32, cam, size)
    dev = torch.from_numpy(frames.astype(np.int16)).cuda()
    fb = cam[0] * cam[1] * 2
    vc = K.camera(*cam)
    eye = None
    rates = {0: [], 1: [], 4: []}
    for rnd in range(3):                                       # alternating: every variant once per round
        for every in (0, 1, 4):
            pipe = PL.SingleGpuPipeline(K.camera(*cam), res, size, dict(trunc_max=wl["trunc_max"], integ_dist=wl["integ_dist"]))
            ctx = pipe.ctx
            # (the stream swings back and forth over 32 frames so that it never jumps)
            idx = lambda k: (k % 62) if (k % 62) < 32 else 62 - (k % 62)
            for k in range(warm + n):
                if k == warm:
                    ctx.sync(); t0 = time.perf_counter()
                pipe.process_frame_device(dev.data_ptr() + idx(k) * fb, k, dev.data_ptr() + idx(k + 1) * fb)
                if every and k % every == 0:
                    ctx.render_view(K.VIEW_SHADED, eye, vc, pipe.inc, P["depth_trunc_min"], wl["trunc_max"])
            ctx.sync()
            rates[every].append(n / (time.perf_counter() - t0))
            st = pipe.stats()
            assert st["frames_lost"] == 0, st
            pipe.close()
    for every, what in ((0, "no view"), (1, "VGA view after every frame"), (4, "VGA view every fourth frame")):
        print(json.dumps(dict(tool="bench_view", leg="stream", what=what, frames=n, device=gpu, fps_runs=[round(v, 1) for v in rates[every]],
                              fps_median=round(med(rates[every]), 1))))


def leg_readback():
    import view_expect as V
    pipe, dev, fb = fused_pipe(6)
    ctx = pipe.ctx
    for k in range(6):
        pipe.process_frame_device(dev.data_ptr() + k * fb, k, None)
    ok, pose, _, _ = pipe.track_result()
    t_view, t_maps, t_conv = [], [], []
    for _ in range(reps):
        ctx.view_model_maps(K.VIEW_NORMALS); ctx.sync()
        t0 = time.perf_counter(); img = ctx.read_view(); t_view.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        mv, mn = ctx.download_map(K.MAP_MODEL_VERTICES), ctx.download_map(K.MAP_MODEL_NORMALS)
        t_maps.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); exp = V.view_bytes(V.VIEW_NORMALS, mv, mn); t_conv.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(tool="bench_view", leg="readback", device=gpu, cols=cam[0], rows=cam[1], view_bytes=int(img.nbytes), map_bytes=int(mv.nbytes + mn.nbytes),
                          same_bytes=bool(np.array_equal(img, exp)), read_view_ms=round(med(t_view), 3), two_download_map_ms=round(med(t_maps), 3),
                          numpy_conversion_ms=round(med(t_conv), 3), reps=reps)))
    pipe.close()


def c2_group(n):
    params = G.stock_params(trunc_max=wl["trunc_max"], integ_dist=wl["integ_dist"])
    return G.Group.local(K.camera(*cam), res, size, [0] + [r[1] for r in PL.slab_ranges(res, n)], params=params)


def group_event_ms(g, fn, n):
    stream = torch.cuda.ExternalStream(g.stream(0))
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def leg_group(n_members, n_frames=12, n=120, warm=20):
    frames, _ = S.make_stream(32, cam, size)
    dev = torch.from_numpy(frames.astype(np.int16)).cuda()
    fb = cam[0] * cam[1] * 2
    vc = K.camera(*cam)
    near, far = P["depth_trunc_min"], wl["trunc_max"]
    # device time: the group and a whole-volume context through the same frames, the view from the last tracked pose
    g = c2_group(n_members)
    whole = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3)
    g.set_pose(S.pose0(size)); whole.set_pose(S.pose0(size))
    inc = g.params.raycast.ray_increment
    for k in range(n_frames):
        g.frame(dev.data_ptr() + k * fb, k)
        whole.set_depth_mm_device(dev.data_ptr() + k * fb)
        whole.preprocess(near, far, P["filter_sigma_pixel"], P["filter_sigma_depth"])
        whole.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
        whole.integrate(None, P["integrate_sdf_trunc"], wl["integ_dist"])
        whole.raycast(None, inc, near, far)
    ok, pose, _, _ = g.track_result(check_lockstep=True)
    for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
        fg = lambda: g.render_view(mode, pose, vc, near, far)
        fw = lambda: whole.render_view(mode, pose, vc, inc, near, far)
        group_event_ms(g, fg, 3); event_ms(whole, fw, 3)
        tg, tw = group_event_ms(g, fg, reps), event_ms(whole, fw, reps)
        same = bool(np.array_equal(g.read_view(), whole.read_view()))
        print(json.dumps(dict(tool="bench_view", leg="group-device", what="kf_group_render_view next to kf_render_view", mode=NAMES[mode], members=n_members,
                              backend="local", res=res, cols=cam[0], rows=cam[1], device=gpu, group_event_us_median=round(1e3 * med(tg), 2),
                              group_event_us_min=round(1e3 * min(tg), 2), whole_event_us_median=round(1e3 * med(tw), 2),
                              whole_event_us_min=round(1e3 * min(tw), 2), same_bytes=same, reps=reps)), flush=True)
    g.close(); whole.close()
    # stream rate of the group with and without a view per frame
    rates = {0: [], 1: []}
    idx = lambda k: (k % 62) if (k % 62) < 32 else 62 - (k % 62)
    for rnd in range(3):
        for every in (0, 1):
            g = c2_group(n_members)
            g.set_pose(S.pose0(size))
            for k in range(warm + n):
                if k == warm:
                    g.sync(); t0 = time.perf_counter()
                g.frame(dev.data_ptr() + idx(k) * fb, k)
                if every:
                    g.render_view(K.VIEW_SHADED, None, vc, near, far)
            g.sync()
            rates[every].append(n / (time.perf_counter() - t0))
            g.track_result(check_lockstep=True)
            assert g.members()[0].stats(observed=False)["frames_lost"] == 0
            g.close()
    for every, what in ((0, "no view"), (1, "VGA merged view after every frame")):
        print(json.dumps(dict(tool="bench_view", leg="group-stream", what=what, members=n_members, backend="local", res=res, frames=n, device=gpu,
                              fps_runs=[round(v, 1) for v in rates[every]], fps_median=round(med(rates[every]), 1))), flush=True)


if leg == "group":
    leg_group(group_n)
for name, fn in (("device", leg_device), ("stream", leg_stream), ("readback", leg_readback)):
    if leg in (name, "all"):
        fn()
