#!/usr/bin/env python3
"""What aligning two maps costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and captured
(the map of tools/bench_map_resample.py), that same map is the source and the store that holds it the destination:
  (a) kf_merge_brick_store_rigid of the source under a 2 degree / 1 voxel transform: the same upload, the same table, the same eight gathers per voxel
      (the store is cleared and the held map written back before every repetition, outside the timed span);
  (b) one evaluation of the sums under the same transform (kf_align_brick_store, max_iter = 0): the upload, the sort of the held keys, one launch, one fold;
  (c) a full alignment from that transform -- the truth is the identity -- with its iteration count, verdict and what is left of the offset.
Wall time (time.perf_counter) around the blocking call, the stream idle before it; one warm-up, then the median of `reps` >= 5 (default 7).  One JSON line per
leg, also collected into the output file.
usage: tools/bench_map_align.py [c2|c4] [reps] [output file, default profiles/map_align_<cfg>.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from hybkinectfu_amd import lib as K, posemath, scene as S
from hybkinectfu_amd.pipeline import SingleGpuPipeline
import bench

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_align_%s.json" % cfg)
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
nb = res // 8
common = dict(tool="bench_map_align", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
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


ctx.brick_store_reserve(2 * nb ** 3)
ctx.shift_volume(8 * (nb // 2), 0, 0)
ctx.brick_store_capture()
keys, t, w, _ = ctx.brick_store()
n = len(keys)
lo, hi = ctx.brick_store_bounds()
centre = np.array([4.0 * (l + h) for l, h in zip(lo, hi)])
r = rotation(2.0, (1, 2, 3))
unit = np.array([1.0, -2.0, 2.0]) / 3.0                           # 1 voxel
OFFSET = np.concatenate([r, (centre - r @ centre + unit).reshape(3, 1)], axis=1)      # 2 degrees about the map's middle, then 1 voxel


def restore_held():
    ctx.brick_store_clear()
    ctx.write_brick_store(keys, t, w)


def wall_ms(fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def timed(fn, before=None):
    out, last = [], None
    for rep in range(reps + 1):
        if before:
            before()
        ms, last = wall_ms(fn)
        if rep:                                                   # (the first one is the warm-up)
            out.append(ms)
    return out, last


def line(leg, ms=None, **kw):
    d = dict(common, leg=leg, **kw)
    if ms is not None:
        d.update(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])
    lines.append(d)
    print(json.dumps(d), flush=True)
    return d


merge = lambda: ctx.merge_brick_store_rigid(keys, t, w, None, OFFSET)
sums = lambda: ctx.align_brick_store(keys, t, w, OFFSET, centre, max_iter=0)
align = lambda: ctx.align_brick_store(keys, t, w, OFFSET, centre, max_iter=25, min_pairs=1000, eps_rot=0.0, eps_trans=0.0)

line("scene", bricks_held=int(n), source_bricks=int(n), bytes_in_per_entry=4096 + 12, offset_deg=2.0, offset_voxels=1.0)
ms, _ = timed(merge, before=restore_held)
held = ctx.brick_store_count()
a = line("a_merge_brick_store_rigid", ms, candidate_bricks=len(K.rigid_brick_keys(keys, OFFSET)), bricks_held_after=int(held[0]), dropped=int(held[1]))
restore_held()
ms, (_, rep) = timed(sums)
b = line("b_sums_once", ms, pairs=int(rep.sums[28]), rms=rep.rms)
ms, (xf, rep) = timed(align)
left = float(np.linalg.norm(xf[:, :3] @ centre + xf[:, 3] - centre))
c = line("c_align_from_2deg_1voxel", ms, iterations=int(rep.iterations), verdict=int(rep.verdict), pairs=int(rep.sums[28]), rms=rep.rms,
         left_voxels=round(left, 6), left_rad=round(posemath.rotation_angle(xf[:, :3], np.eye(3)), 9))
line("ratios", b_over_a=round(b["ms"] / a["ms"], 4), c_over_b=round(c["ms"] / b["ms"], 4))
with open(out_path, "w") as f:
    for d in lines:
        f.write(json.dumps(d) + "\n")
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
