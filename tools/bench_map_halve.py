#!/usr/bin/env python3
"""What halving a map costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and captured (the
map of tools/bench_map_merge.py), that map goes
  (a) through kf_merge_brick_store into an empty store of the same context: the merge there was, with the same upload;
  (b) through kf_merge_brick_store_halved into an empty store of a second context of half the resolution (checked once against (c), bit for bit);
  (c) through the numpy restatement of (b) on the host;
  (d) kf_marching_cubes_map over the map as fused and over the halved one, each with its window placed where the recording window stood: time and
      triangle count.
Before every repetition the store is cleared (and for (d) the triangle buffer), outside the timed span.  Wall time (time.perf_counter) around the blocking
call, the stream idle before it; one warm-up, then the median of `reps` >= 5 (default 7; (c): 3).  One JSON line per leg, also collected into the output file.
usage: tools/bench_map_halve.py [c2|c4] [reps] [output file, default profiles/map_halve_<cfg>.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from hybkinectfu_amd import lib as K, scene as S
from hybkinectfu_amd.pipeline import SingleGpuPipeline
import bench

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_halve_%s.json" % cfg)
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
nb = res // 8
common = dict(tool="bench_map_halve", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []
MAX_TRIS = 4000000

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
ctx.brick_store_reserve(2 * nb ** 3)
ctx.shift_volume(8 * (nb // 2), 0, 0)
ctx.brick_store_capture()
keys, t, w, _ = ctx.brick_store()
n = len(keys)
ncoarse = len(K.halved_brick_keys(keys))
# the fine map alone, in a context with a triangle buffer, and the coarse context
fine = K.Context(K.camera(*cam), res, size, wl.get("max_weight", S.STOCK["volume_max_weight"]), max_triangles=MAX_TRIS)
coarse = K.Context(K.camera(*cam), res // 2, size, wl.get("max_weight", S.STOCK["volume_max_weight"]), max_triangles=MAX_TRIS)
fine.brick_store_reserve(n)
coarse.brick_store_reserve(ncoarse)


def np_halve(keys, t, w):
    """the rule of kf_merge_brick_store_halved without colour (include/hybkf.h), float32, one rounded operation per operation; sorted by (z, y, x)"""
    f32 = np.float32
    at = {tuple(k): i for i, k in enumerate(keys.tolist())}
    ck = np.unique(keys.astype(np.int64) >> 1, axis=0)
    ck = ck[np.lexsort((ck[:, 0], ck[:, 1], ck[:, 2]))]
    child = lambda a, i: a.reshape(8, 2, 8, 2, 8, 2)[:, i >> 2, :, (i >> 1) & 1, :, i & 1]
    ok, ot, ow = [], [], []
    for kc in ck.tolist():
        bt, bw = np.zeros((16, 16, 16), f32), np.zeros((16, 16, 16), f32)
        for d in range(8):
            dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
            i = at.get((2 * kc[0] + dx, 2 * kc[1] + dy, 2 * kc[2] + dz))
            if i is not None:
                bt[8 * dz:8 * dz + 8, 8 * dy:8 * dy + 8, 8 * dx:8 * dx + 8], bw[8 * dz:8 * dz + 8, 8 * dy:8 * dy + 8, 8 * dx:8 * dx + 8] = t[i], w[i]
        obs = bw > 0
        cs = [child(np.where(obs, bt, f32(0)), i) for i in range(8)]
        s = ((cs[0] + cs[1]) + (cs[2] + cs[3])) + ((cs[4] + cs[5]) + (cs[6] + cs[7]))
        cnt = sum(child(obs, i).astype(np.int64) for i in range(8))
        wm = np.full((8, 8, 8), np.inf, f32)
        for i in range(8):
            wm = np.where(child(obs, i), np.minimum(wm, child(bw, i)), wm)
        hw = np.where(cnt > 0, wm, f32(0))
        if np.any(hw > 0):
            ok.append(kc); ot.append(np.where(cnt > 0, s / np.maximum(cnt, 1).astype(f32), f32(0))); ow.append(hw)
    return np.array(ok, np.int32).reshape(-1, 3), np.stack(ot), np.stack(ow)


def wall_ms(c, fn):
    c.sync()
    t0 = time.perf_counter()
    fn()
    c.sync()
    return (time.perf_counter() - t0) * 1e3


def timed(c, fn, before=None, reps=reps):
    out = []
    for rep in range(reps + 1):
        if before:
            before()
        ms = wall_ms(c, fn)
        if rep:                                                   # (the first one is the warm-up)
            out.append(ms)
    return out


def line(leg, ms=None, **kw):
    d = dict(common, leg=leg, **kw)
    if ms is not None:
        d.update(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])
    lines.append(d)
    print(json.dumps(d), flush=True)
    return d


def sorted_store(c):
    k, a, b, _ = c.brick_store()
    o = np.lexsort((k[:, 0], k[:, 1], k[:, 2]))
    return k[o], a[o].view(np.uint32), b[o].view(np.uint32)


line("scene", bricks_held=int(n), coarse_candidates=int(ncoarse), bytes_in_per_entry=4096 + 12)
ms = timed(fine, lambda: fine.merge_brick_store(keys, t, w), before=fine.brick_store_clear)
a = line("a_merge_brick_store_into_empty", ms, bricks_after=int(fine.brick_store_count()[0]), dropped=int(fine.brick_store_count()[1]))
ms = timed(coarse, lambda: coarse.merge_brick_store_halved(keys, t, w), before=coarse.brick_store_clear)
got = sorted_store(coarse)
b = line("b_merge_brick_store_halved_into_empty", ms, bricks_after=int(coarse.brick_store_count()[0]), dropped=int(coarse.brick_store_count()[1]))
host = []
for rep in range(3):
    t0 = time.perf_counter()
    want = np_halve(keys, t, w)
    host.append((time.perf_counter() - t0) * 1e3)
same = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1].view(np.uint32)) and np.array_equal(got[2], want[2].view(np.uint32))
c = line("c_numpy_restatement_on_the_host", host, same_store_as_b=bool(same))
tris = {}
for name, cx, r in (("fine", fine, res), ("halved", coarse, res // 2)):
    cx.place_window(8 * (r // 16), 0, 0)                          # where the recording window stood: a key inside an empty window would be shadowed by it
    thr = 300 * size / r
    ms = timed(cx, lambda: cx.marching_cubes_map(thr), before=cx.clear_triangles)
    tris[name] = line("d_marching_cubes_map_" + name, ms, resolution_of_map=r, triangles=int(len(cx.triangles())))
line("ratios", b_over_a=round(b["ms"] / a["ms"], 4), b_over_c=round(b["ms"] / c["ms"], 6), d_halved_over_fine_ms=round(tris["halved"]["ms"] / tris["fine"]["ms"], 4),
     d_halved_over_fine_triangles=round(tris["halved"]["triangles"] / max(1, tris["fine"]["triangles"]), 4))
with open(out_path, "w") as f:
    for d in lines:
        f.write(json.dumps(d) + "\n")
fine.close(); coarse.close()
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
