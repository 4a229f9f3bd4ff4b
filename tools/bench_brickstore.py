#!/usr/bin/env python3
"""The brick store's cost: after 150 fused frames of Scene S, time kf_shift_volume by one and by four bricks along each axis
  (a) without a store -- the path every context took before the store existed;
  (b) with a store reserved while nothing observed leaves (the shift's sign is chosen so that only empty brick layers leave, where there are any);
  (c) with the window first moved so that the scene's first observed brick layer lies at the window's edge: the shift evicts N observed bricks;
  (d) the shift back, which restores them.
One JSON line per leg, with N and the bytes the store's passes copied.  usage: tools/bench_brickstore.py [c2|c4] [reps]
HIP events on the context's stream, one warm-up, then the median of `reps` >= 5 (default 7).  Between two timed shifts of (a) and (b) the volume is
shifted back (untimed); (c) and (d) are timed as one pair per repetition, the store cleared before each pair so that every (c) inserts at first sight."""
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
SHIFTS = [tuple(8 * n if k == a else 0 for k in range(3)) for n in (1, 4) for a in range(3)]
common = dict(tool="bench_brickstore", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)
BRICK_BYTES = 4096 + 8 + 8                                        # (tsdf, weight) pairs, the deferred-weight word, the key (no colour plane in this workload)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(d):
    back = tuple(-x for x in d)
    ctx.shift_volume(*d); ctx.shift_volume(*back); ctx.sync()     # warm-up
    out = []
    for _ in range(reps):
        out.append(event_ms(lambda: ctx.shift_volume(*d)))
        ctx.shift_volume(*back); ctx.sync()
    return out


def line(leg, d, ms, **kw):
    print(json.dumps(dict(common, leg=leg, shift=list(d), ms=round(med(ms), 4), ms_all=[round(x, 4) for x in ms], **kw)), flush=True)


# which bricks the scene has touched: everything leaves into a store and comes back; the store's keys are the observed bricks
ctx.brick_store_reserve(nb ** 3 // 2)
ctx.shift_volume(8 * nb, 0, 0); ctx.shift_volume(-8 * nb, 0, 0)
held, dropped, restored = ctx.brick_store_count()
assert dropped == 0 and restored == held, (held, dropped, restored)
keys = ctx.brick_store()[0]
lo, hi = keys.min(axis=0), keys.max(axis=0)
cap = 2 * held


def idle(d):
    """d, or -d, whichever makes only empty brick layers leave (d itself when neither does: the leg then reports what it evicted)"""
    axis = [k for k in range(3) if d[k]][0]
    n = d[axis] // 8
    return d if lo[axis] >= n or hi[axis] >= nb - n else tuple(-x for x in d)


print(json.dumps(dict(common, leg="scene", observed_bricks=int(held), bricks_total=nb ** 3, first_observed_brick=[int(x) for x in lo],
                      last_observed_brick=[int(x) for x in hi], store_bricks=cap)), flush=True)

base = {}
for d in SHIFTS:                                                  # (a) no store
    ctx.brick_store_reserve(0)
    a = timed(idle(d))
    base[d] = med(a)
    line("a_no_store", idle(d), a, evicted=0, store_bytes=0)
for d in SHIFTS:                                                  # (b) a store, nothing observed leaves
    ctx.brick_store_reserve(cap)
    b = timed(idle(d))
    n = ctx.brick_store_count()[0]
    line("b_store_idle", idle(d), b, evicted=int(n), store_bytes=int(n) * BRICK_BYTES, over_a=round(med(b) / base[d], 4))
for d in SHIFTS:                                                  # (c) + (d): the scene's first observed layer at the window's edge
    axis = [k for k in range(3) if d[k]][0]
    pre = tuple(8 * int(lo[k]) if k == axis else 0 for k in range(3))
    back = tuple(-x for x in d)
    ctx.brick_store_reserve(cap)
    ctx.shift_volume(*pre)                                        # bricks [0, lo) are empty: nothing is lost on the way
    c_ms, d_ms, n_ev, n_re = [], [], 0, 0
    for rep in range(reps + 1):
        ctx.brick_store_clear(); ctx.sync()
        c1 = event_ms(lambda: ctx.shift_volume(*d))
        d1 = event_ms(lambda: ctx.shift_volume(*back))
        n_ev, dr, n_re = ctx.brick_store_count()
        assert dr == 0 and n_re == n_ev, (n_ev, dr, n_re)
        if rep:                                                   # (the first pair is the warm-up)
            c_ms.append(c1); d_ms.append(d1)
    ctx.shift_volume(*[-x for x in pre])
    line("c_evict", d, c_ms, evicted=int(n_ev), store_bytes=int(n_ev) * BRICK_BYTES, over_a=round(med(c_ms) / base[d], 4), pre_shift=list(pre))
    line("d_restore", back, d_ms, restored=int(n_re), store_bytes=int(n_re) * BRICK_BYTES, over_a=round(med(d_ms) / base[d], 4), pre_shift=list(pre))
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
