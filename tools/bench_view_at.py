#!/usr/bin/env python3
"""What a viewer frame of the map costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x (so the
surface in the half that left lives in the store alone), render the tracking camera's view
  (a) kf_render_view of the current window;
  (b) kf_render_view_at at the window's own origin: the same picture through the indirection table -- the price of the indirection and of the resolve pass;
      b_resolve: the same call with a 1 x 1 camera -- the clears, the resolve pass over all bricks and a march of one ray: an upper estimate of the resolve's
      share of (b);
  (c) kf_render_view_at of the OLD place, half a window away, nothing moved;
  (d) the only way there was: kf_shift_volume back to the old place, kf_render_view, kf_shift_volume forth again.
One JSON line per leg.  usage: tools/bench_view_at.py [c2|c4] [reps]
HIP events on the context's stream, one warm-up, then the median of `reps` >= 5 (default 7).  (a) and (b), (c) and (d) are checked to give the same
bytes before they are timed."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hybkinectfu_amd import lib as K, scene as S
from hybkinectfu_amd.pipeline import SingleGpuPipeline
import bench

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
med = statistics.median
nb = res // 8
P = S.STOCK
common = dict(tool="bench_view_at", config=wl["name"], resolution=res, size_m=size, camera=[cam[0], cam[1]], device=torch.cuda.get_device_name(0), reps=reps)

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)
inc, near, far = pipe.inc, P["depth_trunc_min"], P["depth_trunc_max"]
view_cam, one_ray = K.camera(*cam), K.camera(1, 1, 0.0, 0.0, cam[4], cam[5])
mode = K.VIEW_SHADED


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn):
    out = []
    for rep in range(reps + 1):
        ctx.sync()
        ms = event_ms(fn)
        if rep:                                                   # (the first one is the warm-up)
            out.append(ms)
    return out


def line(leg, ms, **kw):
    print(json.dumps(dict(common, leg=leg, ms=round(med(ms), 4), ms_all=[round(x, 4) for x in ms], **kw)), flush=True)


def moved(pose, d):
    out = np.array(pose, np.float32)
    for i in range(3):
        out[i, 3] = np.float32(out[i, 3]) - np.float32(d[i]) * np.float32(size / res)
    return out


ctx.brick_store_reserve(nb ** 3)
old = ctx.volume_origin()
pose_old = ctx.track_result()[1]                                  # the tracked pose, in the old place's coordinates
d = (8 * (nb // 2), 0, 0)
back = tuple(-x for x in d)
ctx.shift_volume(*d)
here = ctx.volume_origin()
pose_here = moved(pose_old, d)                                    # the same viewpoint seen from the window where it stands now
held, dropped, _ = ctx.brick_store_count()
assert held > 0 and dropped == 0, (held, dropped)
print(json.dumps(dict(common, leg="scene", bricks_total=nb ** 3, shift=list(d), bricks_in_store=int(held))), flush=True)


def leg_a():
    ctx.render_view(mode, pose_here, view_cam, inc, near, far)


def leg_b():
    ctx.render_view_at(mode, here, pose_here, view_cam, inc, near, far)


def leg_b_resolve():
    ctx.render_view_at(mode, here, pose_here, one_ray, inc, near, far)


def leg_c():
    ctx.render_view_at(mode, old, pose_old, view_cam, inc, near, far)


def leg_d():
    ctx.shift_volume(*back)
    ctx.render_view(mode, pose_old, view_cam, inc, near, far)
    ctx.shift_volume(*d)


def hits(img):
    return int((img[..., 3] == 255).sum())


leg_a(); ia = ctx.read_view()
leg_b(); ib = ctx.read_view()
assert np.array_equal(ia, ib), (hits(ia), hits(ib))
leg_c(); ic = ctx.read_view()
leg_d(); idd = ctx.read_view()
assert np.array_equal(ic, idd) and hits(ic) > 0, (hits(ic), hits(idd))
a = timed(leg_a)
line("a_render_view", a, hits=hits(ia))
b = timed(leg_b)
br = timed(leg_b_resolve)
line("b_view_at_same_window", b, hits=hits(ib), b_over_a=round(med(b) / med(a), 3))
line("b_resolve", br, share_of_b=round(med(br) / med(b), 3))
c = timed(leg_c)
dd = timed(leg_d)
line("c_view_at_old_place", c, hits=hits(ic), frame=list(old))
line("d_shift_view_shift", dd, hits=hits(idd), frame=list(old), c_over_d=round(med(c) / med(dd), 4))
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
