#!/usr/bin/env python3
"""What relocalising a frame costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and captured
(the map of tools/bench_map_query.py), the level-2 vertices of the next VGA frame are scored under a lattice of candidate poses around the tracked one.
  (a) kf_map_score_poses_device for 5^6 = 15 625 candidates (translation steps of one truncation, rotation steps of atan(truncation / median depth));
  (b) the only way there was to get the same counts: the positions formed on the host, kf_map_sample (host form), a numpy classification -- timed by the
      host clock for a slice of 64 candidates and stated per candidate; the counts of the slice are checked against (a)'s;
  (c) one kf_map_pose_sums over the 16 best candidates (the host form: its allocation and copies are part of it), by HIP events around the call and by the
      host clock;
  (d) HybKinectfu::relocalise end to end, by the host clock: an App of the same configuration fuses the same 150 frames, then the next frame is relocalised
      with the defaults (5^6 candidates, at most 4 096 points of the coarsest level, the best 16 refined) from the pose it holds (repeats start from the pose the one before found).
One JSON line per leg, also collected into the output file.  usage: tools/bench_map_reloc.py [c2|c4] [reps] [output file, default profiles/map_reloc_<cfg>.json]
HIP events on the context's stream around (a), one warm-up, then the median of `reps` >= 5 (default 7).  Nothing is asserted on any time or ratio."""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_reloc_%s.json" % cfg)
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
P = S.STOCK
N_UNIQUE = 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
med = statistics.median
nb = res // 8
f32, f64 = np.float32, np.float64
BAND, SLICE, TOP = 0.5, 64, 16
common = dict(tool="bench_map_reloc", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device(), max_triangles=0)
ctx = pipe.ctx
for k in range(150):
    pipe.process_frame_device(ptr(k), k, ptr(k + 1))
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)


def line(leg, ms=None, **kw):
    d = dict(common, leg=leg, **kw)
    if ms is not None:
        d.update(ms=round(med(ms), 4), ms_all=[round(x, 4) for x in ms])
    lines.append(d)
    print(json.dumps(d), flush=True)
    return d


def host_ms(fn):
    out = []
    for rep in range(reps + 1):
        ctx.sync()
        t = time.perf_counter(); fn(); ctx.sync()
        if rep:
            out.append(1e3 * (time.perf_counter() - t))
    return out


ctx.brick_store_reserve(2 * nb ** 3)
ctx.shift_volume(8 * (nb // 2), 0, 0)
ctx.brick_store_capture()
ctx.raycast(None, pipe.inc, P["depth_trunc_min"], pipe.trunc_max)
origin = np.array(ctx.volume_origin(), f64)
cell = f32(size) / f32(res)
trunc_vox = float(f32(P["integrate_sdf_trunc"]) / cell)          # the truncation in voxels

# the points: the level-2 vertices of the frame the pipeline preprocessed last, valid ones, camera frame, voxels
verts = ctx.download_map(K.MAP_NEW_VERTICES, 2).reshape(-1, 4)
valid = verts[:, 2] != 0
pts = np.ascontiguousarray((verts[valid, :3].astype(f64) / float(cell)).astype(f32))
median_depth = float(np.median(pts[:, 2]))

# the lattice around the tracked pose: translation outermost, the first index slowest, the last rotation index fastest
pose = ctx.track_result()[1].astype(f64)
Rc, tc = pose[:3, :3], pose[:3, 3] / float(cell) + origin
rot_step = float(np.arctan(trunc_vox / median_depth))
idx = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 6, indexing="ij"), axis=-1).reshape(-1, 6)


def exp_so3(w):
    th = np.linalg.norm(w, axis=1)[:, None, None]
    W = np.zeros((len(w), 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        A, B = np.where(th > 0, np.sin(th) / th, 1.0), np.where(th > 0, (1 - np.cos(th)) / th ** 2, 0.5)
    return np.eye(3) + A * W + B * (W @ W)


poses = np.zeros((len(idx), 3, 4))
poses[:, :, :3] = Rc @ exp_so3(idx[:, 3:] * rot_step)
poses[:, :, 3] = tc + idx[:, :3] * trunc_vox
K_POSES, N_PTS = len(poses), len(pts)

gpu = torch.device("cuda")
d_pts, d_poses = torch.from_numpy(pts).to(gpu), torch.from_numpy(poses).to(gpu)
d_sc = torch.zeros(K_POSES * 24, dtype=torch.uint8, device=gpu)
torch.cuda.synchronize()


def score():
    ctx.map_score_poses_device(N_PTS, d_pts.data_ptr(), K_POSES, d_poses.data_ptr(), BAND, d_sc.data_ptr())


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


a_ms = []
for rep in range(reps + 1):
    ctx.sync()
    ms = event_ms(score)
    if rep:
        a_ms.append(ms)
sc = d_sc.cpu().numpy().view(K.POSE_SCORE_DTYPE)
key = 2 * sc["n_in"].astype(np.int64) - sc["n_obs"]
order = np.lexsort((np.arange(K_POSES), sc["sum_q"], -key))
best = int(order[0])

sl = order[:SLICE // 2].tolist() + list(range(0, K_POSES, K_POSES // (SLICE // 2)))[:SLICE // 2]
p64 = pts.astype(f64)


def parent_way():
    out = np.zeros(len(sl), K.POSE_SCORE_DTYPE)
    w = np.stack([np.stack([((poses[k, j, 0] * p64[:, 0] + poses[k, j, 1] * p64[:, 1]) + poses[k, j, 2] * p64[:, 2]) + poses[k, j, 3] for j in range(3)], axis=1) for k in sl])
    s = ctx.map_sample(w.reshape(-1, 3), want=("tsdf", "weight"))
    t, seen = s["tsdf"].reshape(len(sl), -1), s["weight"].reshape(len(sl), -1) > 0
    a = np.abs(t)
    inb = seen & (a < f32(BAND))
    behind = seen & ~inb & (t < 0)
    q = np.where(seen, (np.minimum(a, f32(1)) * f32(65536)).astype(np.uint32), 0).astype(np.uint64)
    out["n_obs"], out["n_in"], out["n_behind"], out["sum_q"] = seen.sum(1), inb.sum(1), behind.sum(1), q.sum(1)
    out["n_free"] = out["n_obs"] - out["n_in"] - out["n_behind"]
    return out


assert parent_way().tobytes() == sc[sl].tobytes(), "the kernel and the sampled classification disagree"
b_ms = host_ms(parent_way)

top = order[:TOP]
centres = np.stack([(p64 @ poses[k, :, :3].T + poses[k, :, 3]).mean(axis=0) for k in top])
sums = ctx.map_pose_sums(pts, poses[top], centres, 1.0)
c_ms = host_ms(lambda: ctx.map_pose_sums(pts, poses[top], centres, 1.0))
c_ev = []
for rep in range(reps + 1):
    ctx.sync()
    ms = event_ms(lambda: ctx.map_pose_sums(pts, poses[top], centres, 1.0))
    if rep:
        c_ev.append(ms)

line("scene", points=N_PTS, candidates=K_POSES, median_depth_voxels=round(median_depth, 2), trans_step_voxels=round(trunc_vox, 4), rot_step_rad=round(rot_step, 6),
     best_index=best, centre_index=K_POSES // 2, best_score={k: int(sc[k][best]) for k in sc.dtype.names}, centre_score={k: int(sc[k][K_POSES // 2]) for k in sc.dtype.names})
a = line("a_score_poses_device", a_ms, candidates=K_POSES, points=N_PTS)
b = line("b_host_positions_map_sample_numpy", b_ms, candidates=len(sl), points=N_PTS, clock="host")
c = line("c_pose_sums_16_poses_host_form", c_ev, poses=TOP, points=N_PTS, pairs_of_the_best=int(sums[0, 28]), clock="HIP events", ms_host_clock=round(med(c_ms), 4))
line("per_candidate", us_a=round(1e3 * a["ms"] / K_POSES, 4), us_b=round(1e3 * b["ms"] / len(sl), 4), b_over_a=round((b["ms"] / len(sl)) / (a["ms"] / K_POSES), 1))
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()

# (d) through the host class: one context at a time, so the pipeline's is closed first
from hybkinectfu_amd import host_app as H
app = H.App(res, size, cam, sdf_trunc=P["integrate_sdf_trunc"], integrate_dist=wl["integ_dist"], trunc_max=wl["trunc_max"])
host_frames = frames.astype(np.uint16)
for k in range(150):
    assert app.process_frame(host_frames[k % N_UNIQUE], k), k
d_ms, rep = [], None
for r in range(reps + 1):
    t = time.perf_counter()
    ok, rep = app.relocalise(host_frames[150 % N_UNIQUE], 150)
    ms = 1e3 * (time.perf_counter() - t)
    assert ok, rep
    if r:
        d_ms.append(ms)
line("d_relocalise_end_to_end", d_ms, clock="host", candidates=rep["candidates"], points=rep["points"], verdict=rep["verdict"], iterations=rep["iterations"],
     refined_score=rep["refined_score"], trans_step_m=round(rep["trans_step"], 5), rot_step_rad=round(rep["rot_step"], 6))
app.close()
line("not_run", what="configurations other than the one named above; no threshold is set on any leg")
with open(out_path, "w") as f:
    for d_ in lines:
        f.write(json.dumps(d_) + "\n")
