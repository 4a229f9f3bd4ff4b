#!/usr/bin/env python3
"""What the map mesh costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted four bricks along x past the scene's
first observed brick layer (bench_brickstore.py's leg c: 982 bricks in the store at C2), extract the model around the OLD place
  (a) the only way there was: kf_shift_volume back to the old place, kf_marching_cubes_region over the whole box, kf_shift_volume forth again;
  (b) kf_marching_cubes_at for the same frame and box, nothing moved;
  (c) the price of the indirection: kf_marching_cubes_at with frame == origin over the whole volume against kf_marching_cubes_region over the whole
      volume, on the same window;
  (d) kf_marching_cubes_map for a walk (four bricks along x, four along y, back to the start): tiles visited, triangles, total time.
One JSON line per leg.  usage: tools/bench_mapmesh.py [c2|c4] [reps]
HIP events on the context's stream, one warm-up, then the median of `reps` >= 5 (default 7); the triangle buffer is cleared (untimed) before every timed
extraction.  (a) and (b) are checked to give the same triangles before they are timed."""
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
thr = 300 * size / res
common = dict(tool="bench_mapmesh", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device(), max_triangles=8_000_000)
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn):
    out = []
    for rep in range(reps + 1):
        ctx.clear_triangles(); ctx.sync()
        ms = event_ms(fn)
        if rep:                                                   # (the first one is the warm-up)
            out.append(ms)
    return out


def line(leg, ms, **kw):
    print(json.dumps(dict(common, leg=leg, ms=round(med(ms), 4), ms_all=[round(x, 4) for x in ms], **kw)), flush=True)


# which bricks the scene has touched (as bench_brickstore.py finds them): everything leaves into a store and comes back
ctx.brick_store_reserve(nb ** 3 // 2)
ctx.shift_volume(8 * nb, 0, 0); ctx.shift_volume(-8 * nb, 0, 0)
held, dropped, restored = ctx.brick_store_count()
assert dropped == 0 and restored == held, (held, dropped, restored)
first = ctx.brick_store()[0].min(axis=0)
cap = 2 * held
ctx.brick_store_reserve(cap)
pre = (8 * int(first[0]), 0, 0)
ctx.shift_volume(*pre)                                            # bricks [0, first) are empty: nothing observed leaves
assert ctx.brick_store_count()[0] == 0
old = ctx.volume_origin()
d = (32, 0, 0)
back = tuple(-x for x in d)
ctx.shift_volume(*d)
in_store = ctx.brick_store_count()[0]
whole = ((0, 0, 0), (res, res, res))
print(json.dumps(dict(common, leg="scene", observed_bricks=int(held), bricks_total=nb ** 3, pre_shift=list(pre), shift=list(d), bricks_in_store=int(in_store))), flush=True)


def leg_a():
    ctx.shift_volume(*back)
    ctx.marching_cubes_region(thr, *whole, flags=K.MC_WORLD)
    ctx.shift_volume(*d)


def leg_b():
    ctx.marching_cubes_at(thr, old, *whole, flags=K.MC_WORLD)


ctx.clear_triangles(); leg_a(); ta = ctx.triangles()
ctx.clear_triangles(); leg_b(); tb = ctx.triangles()
assert len(ta) > 0 and np.array_equal(ta.view(np.uint8), tb.view(np.uint8)), (len(ta), len(tb))
a = timed(leg_a)
line("a_shift_region_shift", a, triangles=len(ta), frame=list(old))
b = timed(leg_b)
line("b_at", b, triangles=len(tb), frame=list(old), work=list(ctx.region_work()), a_over_b=round(med(a) / med(b), 3))

here = ctx.volume_origin()
c_region = timed(lambda: ctx.marching_cubes_region(thr, *whole, flags=K.MC_WORLD))
n_region, w_region = len(ctx.triangles()), ctx.region_work()
c_at = timed(lambda: ctx.marching_cubes_at(thr, here, *whole, flags=K.MC_WORLD))
n_at, w_at = len(ctx.triangles()), ctx.region_work()
assert n_region == n_at
line("c_region_same_window", c_region, triangles=n_region, work=list(w_region))
line("c_at_same_window", c_at, triangles=n_at, work=list(w_at), at_over_region=round(med(c_at) / med(c_region), 3))

ctx.shift_volume(0, 32, 0)                                        # (d) the walk goes on: four bricks along y, then back to the start
ctx.shift_volume(-32, -32, 0)
tiles = [0]


def leg_d():
    tiles[0] = ctx.marching_cubes_map(thr)


dm = timed(leg_d)
line("d_map", dm, tiles=int(tiles[0]), triangles=len(ctx.triangles()), bricks_in_store=int(ctx.brick_store_count()[0]), window_origin=list(ctx.volume_origin()))
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
