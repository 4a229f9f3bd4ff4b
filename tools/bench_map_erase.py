#!/usr/bin/env python3
"""What erasing from the map costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and captured
(the map of tools/bench_map_merge.py), a box is erased from the store: a half space along x with its face inside a brick, so that about half the bricks go
and one layer of bricks is cut.
  (a) the only way there was: kf_read_brick_store of the whole map, the same erase in numpy on the host, kf_brick_store_clear, kf_write_brick_store of what
      is left (checked once to leave the same store as (b), bit for bit);
  (b) kf_brick_store_erase_box with that box;
  (c) kf_brick_store_erase_box with a box beside the map: nothing is removed -- the mark pass, the scan, the table rebuilt and the two reads of the counts;
  (d) kf_brick_store_erase_weak at the median of the bricks' greatest weights;
  (e) kf_refill_window after (b).
Before every repetition of (a), (b) and (d) the store is cleared and the map written back, outside the timed span.
One JSON line per leg, also collected into the output file.  usage: tools/bench_map_erase.py [c2|c4] [reps] [output file, default profiles/map_erase_<cfg>.json]
HIP events on the context's stream around each leg (host work between the events included: every leg but (e) blocks on the host), one warm-up, then the
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_erase_%s.json" % cfg)
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
common = dict(tool="bench_map_erase", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())
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
# the box: everything below a plane x = const that lies three voxels inside the median brick layer
face = int(8 * np.median(keys[:, 0]) + 3)
BIG = (1 << 31) - 1
lo, hi = (-BIG - 1, -BIG - 1, -BIG - 1), (face, BIG, BIG)
beside_lo = tuple(int(8 * (v + 4)) for v in keys.max(axis=0))
beside_hi = tuple(v + 64 for v in beside_lo)
top = w.reshape(n, -1).max(axis=1)
weak = float(np.median(top))
z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")


def np_erase(hk, ht, hw):
    """the box erase on the host, mode inside: (keys, tsdf, weight) of what is left"""
    clear = (hk[:, 0].astype(np.int64)[:, None, None, None] * 8 + x[None]) < face
    t2, w2 = np.where(clear, f32(0), ht), np.where(clear, f32(0), hw)
    left = (w2 > 0).reshape(len(hk), -1).any(axis=1)
    return hk[left], t2[left], w2[left]


def restore_held():
    ctx.brick_store_clear()
    ctx.write_brick_store(keys, t, w)


def parents_way():
    hk, ht, hw, _ = ctx.brick_store()
    k2, t2, w2 = np_erase(hk, ht, hw)
    ctx.brick_store_clear()
    ctx.write_brick_store(k2, t2, w2)


def sorted_store():
    k, a, b, _ = ctx.brick_store()
    o = np.lexsort((k[:, 0], k[:, 1], k[:, 2]))
    return k[o], a[o].view(np.uint32), b[o].view(np.uint32)


results = {}


def erase_box():
    results["box"] = ctx.brick_store_erase_box(lo, hi, K.ERASE_INSIDE)


def erase_beside():
    results["beside"] = ctx.brick_store_erase_box(beside_lo, beside_hi, K.ERASE_INSIDE)


def erase_weak():
    results["weak"] = ctx.brick_store_erase_weak(weak)


restore_held(); erase_box(); got_b = sorted_store()
restore_held(); parents_way(); got_a = sorted_store()
assert all(np.array_equal(p, q) for p, q in zip(got_a, got_b)), "kf_brick_store_erase_box and the host erase disagree"
cut = int(np.count_nonzero((keys[:, 0] == face >> 3)))
line("scene", bricks_held=int(n), box_face_x_vox=face, bricks_in_the_cut_layer=cut, weak_min_weight=weak, bytes_per_brick=4096 + 8 + 8)
a = line("a_read_out_numpy_erase_clear_write", timed(parents_way, before=restore_held), bricks=int(n), bricks_left=int(len(got_a[0])))
b = line("b_erase_box", timed(erase_box, before=restore_held), bricks=int(n), bricks_removed=int(results["box"][0]), voxels_cleared=int(results["box"][1]))
restore_held()
c = line("c_erase_box_beside_the_map", timed(erase_beside), bricks=int(n), bricks_removed=int(results["beside"][0]))
d = line("d_erase_weak", timed(erase_weak, before=restore_held), bricks=int(n), min_weight=weak, bricks_removed=int(results["weak"]))
restore_held(); erase_box()
e = line("e_refill_window", timed(ctx.refill_window), bricks_in_store=int(ctx.brick_store_count()[0]), bricks_total=nb ** 3)
line("ratios", b_over_a=round(b["ms"] / a["ms"], 5), c_over_b=round(c["ms"] / b["ms"], 4), d_over_b=round(d["ms"] / b["ms"], 4))
line("not_run", what="configurations other than the one named above; a colour context; a store filled to its capacity; no threshold is set on any leg")
with open(out_path, "w") as f:
    for d_ in lines:
        f.write(json.dumps(d_) + "\n")
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
