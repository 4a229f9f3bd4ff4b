#!/usr/bin/env python3
"""What merging a map costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and captured (the
map of tools/bench_map_file.py), a second map of the same size is merged in: the first map's bricks, in another order, under keys translated by
two bricks along y, so that a known share of the keys collide with held ones and the rest are new.
  (a) kf_merge_brick_store of the whole second map;
  (b) the only way there was to get the same store: kf_read_brick_store of the held map, the same average in numpy on the host for the colliding keys,
      kf_write_brick_store of the result (checked once to leave the same store as (a), bit for bit);
  (c) kf_write_brick_store of the same entries: the copy-only floor (later write wins);
  (d) kf_refill_window: clears and the restore of all bricks.
Before every repetition of (a), (b) and (c) the store is cleared and the held map written back, outside the timed span.
One JSON line per leg, also collected into the output file.  usage: tools/bench_map_merge.py [c2|c4] [reps] [output file, default profiles/map_merge_<cfg>.json]
HIP events on the context's stream around each leg (host work between the events included: every leg but (d) blocks on the host), one warm-up, then the
median of `reps` >= 5 (default 7)."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from hybkinectfu_amd import lib as K, scene as S
from hybkinectfu_amd.pipeline import SingleGpuPipeline
import bench

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_merge_%s.json" % cfg)
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
med = statistics.median
nb = res // 8
f32 = np.float32
common = dict(tool="bench_map_merge", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)
max_weight = float(wl.get("max_weight", S.STOCK["volume_max_weight"]))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, before=None):
    out = []
    for rep in range(reps + 1):
        if before:
            before()
        ctx.sync()
        ms = event_ms(fn)
        if rep:                                                   # (the first one is the warm-up)
            out.append(ms)
    return out


def line(leg, ms=None, **kw):
    d = dict(common, leg=leg, **kw)
    if ms is not None:
        d.update(ms=round(med(ms), 4), ms_all=[round(x, 4) for x in ms])
    lines.append(d)
    print(json.dumps(d), flush=True)
    return d


ctx.brick_store_reserve(2 * nb ** 3)
ctx.shift_volume(8 * (nb // 2), 0, 0)
ctx.brick_store_capture()
keys, t, w, _ = ctx.brick_store()
n = len(keys)
order = np.random.default_rng(1).permutation(n)
keys2 = np.ascontiguousarray(keys[order] + np.array([0, 2, 0], np.int32))
t2, w2 = np.ascontiguousarray(t[np.roll(order, 1)]), np.ascontiguousarray(w[np.roll(order, 1)])   # other bricks' contents under the keys
held_at = {tuple(k): i for i, k in enumerate(keys.tolist())}
hit = np.array([held_at.get(tuple(k), -1) for k in keys2.tolist()])
colliding = int(np.count_nonzero(hit >= 0))
line("scene", bricks_held=int(n), bricks_merged=int(n), colliding_keys=colliding, colliding_share=round(colliding / n, 4),
     bytes_in_per_entry=4096 + 12, max_weight=max_weight)


def restore_held():
    ctx.brick_store_clear()
    ctx.write_brick_store(keys, t, w)


def merge():
    ctx.merge_brick_store(keys2, t2, w2)


def np_rule(ta, wa, tb, wb):
    take, blend = (wb > 0) & ~(wa > 0), (wb > 0) & (wa > 0)
    s = np.where(blend, wa + wb, f32(1))
    return (np.where(blend, (ta * wa + tb * wb) / s, np.where(take, tb, ta)),
            np.where(blend, np.minimum(wa + wb, f32(max_weight)), np.where(take, wb, wa)))


def parents_way():
    """read the held map out, average the colliding bricks on the host, write the result: new keys are added, held ones overwritten with the average"""
    hk, ht, hw, _ = ctx.brick_store()
    at = {tuple(k): i for i, k in enumerate(hk.tolist())}
    idx = np.array([at.get(tuple(k), -1) for k in keys2.tolist()])
    mt, mw = t2.copy(), w2.copy()
    c = idx >= 0
    mt[c], mw[c] = np_rule(ht[idx[c]], hw[idx[c]], t2[c], w2[c])
    ctx.write_brick_store(keys2, mt, mw)


def write():
    ctx.write_brick_store(keys2, t2, w2)


def sorted_store():
    k, a, b, _ = ctx.brick_store()
    o = np.lexsort((k[:, 0], k[:, 1], k[:, 2]))
    return k[o], a[o].view(np.uint32), b[o].view(np.uint32)


restore_held(); merge(); got_a = sorted_store()
restore_held(); parents_way(); got_b = sorted_store()
assert all(np.array_equal(x, y) for x, y in zip(got_a, got_b)), "kf_merge_brick_store and the host average disagree"
a = line("a_merge_brick_store", timed(merge, before=restore_held), bricks=int(n), colliding_keys=colliding)
b = line("b_read_out_numpy_average_write", timed(parents_way, before=restore_held), bricks=int(n), colliding_keys=colliding)
c = line("c_write_brick_store", timed(write, before=restore_held), bricks=int(n))
restore_held(); merge()
d = line("d_refill_window", timed(ctx.refill_window), bricks_in_store=int(ctx.brick_store_count()[0]), bricks_total=nb ** 3)
line("ratios", a_over_b=round(a["ms"] / b["ms"], 4), a_over_c=round(a["ms"] / c["ms"], 4))
with open(out_path, "w") as f:
    for d in lines:
        f.write(json.dumps(d) + "\n")
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
