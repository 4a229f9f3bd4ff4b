#!/usr/bin/env python3
"""What merging a map under a rigid transform costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width
along x and captured (the map of tools/bench_map_merge.py), that same map is merged into the store that holds it:
  (a) kf_merge_brick_store, keys as they are: every key collides (the only merge there was);
  (b) kf_merge_brick_store_rigid with the identity: the same result through the resampling kernel (checked once, bit for bit);
  (c) kf_merge_brick_store_rigid with a rotation of 20 degrees about (1, 2, 3) and the translation (2.3, -1.7, 0.4) voxels;
  (d) of (c)'s host part what the ABI exposes on its own: kf_rigid_brick_keys (the candidate boxes, the sort, the unique list).  The source table and the
      candidates' base corners are built inside the blocking call and are part of (b) and (c) only.
Before every repetition the store is cleared and the held map written back, outside the timed span.  Wall time (time.perf_counter) around the blocking call,
the stream idle before it; one warm-up, then the median of `reps` >= 5 (default 7).  One JSON line per leg, also collected into the output file.
usage: tools/bench_map_resample.py [c2|c4] [reps] [output file, default profiles/map_resample_<cfg>.json]"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_resample_%s.json" % cfg)
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
nb = res // 8
common = dict(tool="bench_map_resample", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0


def rotation(deg, axis):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(a) * np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * np.outer(k, k)


IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
GENERAL = np.concatenate([rotation(20, (1, 2, 3)), np.array([[2.3], [-1.7], [0.4]])], axis=1)

ctx.brick_store_reserve(2 * nb ** 3)
ctx.shift_volume(8 * (nb // 2), 0, 0)
ctx.brick_store_capture()
keys, t, w, _ = ctx.brick_store()
n = len(keys)


def restore_held():
    ctx.brick_store_clear()
    ctx.write_brick_store(keys, t, w)


def wall_ms(fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed(fn, before=None):
    out, held = [], None
    for rep in range(reps + 1):
        if before:
            before()
        ms = wall_ms(fn)
        if rep:                                                   # (the first one is the warm-up)
            out.append(ms)
        held = ctx.brick_store_count()
    return out, held


def line(leg, ms=None, **kw):
    d = dict(common, leg=leg, **kw)
    if ms is not None:
        d.update(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])
    lines.append(d)
    print(json.dumps(d), flush=True)
    return d


def sorted_store():
    k, a, b, _ = ctx.brick_store()
    o = np.lexsort((k[:, 0], k[:, 1], k[:, 2]))
    return k[o], a[o].view(np.uint32), b[o].view(np.uint32)


merge = lambda: ctx.merge_brick_store(keys, t, w)
rigid_identity = lambda: ctx.merge_brick_store_rigid(keys, t, w, None, IDENTITY)
rigid_general = lambda: ctx.merge_brick_store_rigid(keys, t, w, None, GENERAL)
host_general = lambda: K.load().kf_rigid_brick_keys(n, K._p(keys), K.rigid_xf(GENERAL), None, 0)

line("scene", bricks_held=int(n), bricks_merged=int(n), bytes_in_per_entry=4096 + 12)
restore_held(); merge(); got_a = sorted_store()
restore_held(); rigid_identity(); got_b = sorted_store()
identical = all(np.array_equal(x, y) for x, y in zip(got_a, got_b))
cand_i, cand_g = len(K.rigid_brick_keys(keys, IDENTITY)), len(K.rigid_brick_keys(keys, GENERAL))
ms, held = timed(merge, before=restore_held)
a = line("a_merge_brick_store", ms, candidate_bricks=int(n), bricks_held_before=int(n), bricks_held_after=int(held[0]), dropped=int(held[1]))
ms, held = timed(rigid_identity, before=restore_held)
b = line("b_rigid_identity", ms, candidate_bricks=cand_i, bricks_held_before=int(n), bricks_held_after=int(held[0]), dropped=int(held[1]), same_store_as_a=bool(identical))
ms, held = timed(rigid_general, before=restore_held)
c = line("c_rigid_20deg_fractional", ms, candidate_bricks=cand_g, bricks_held_before=int(n), bricks_held_after=int(held[0]), dropped=int(held[1]))
ms, _ = timed(host_general)
d = line("d_host_candidate_list_of_c", ms, candidate_bricks=cand_g)
line("ratios", b_over_a=round(b["ms"] / a["ms"], 4), c_over_a=round(c["ms"] / a["ms"], 4), d_over_c=round(d["ms"] / c["ms"], 4))
with open(out_path, "w") as f:
    for d in lines:
        f.write(json.dumps(d) + "\n")
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
