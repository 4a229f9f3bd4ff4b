#!/usr/bin/env python3
"""What querying the map costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and captured
(the map of tools/bench_map_merge.py and tools/bench_map_erase.py), points are sampled and rays are cast through window and store where they lie.
  (a) kf_map_sample_device at 2^20 random points in the map's bounds (most of them unobserved: bricks nobody holds cost a probe and no load);
  (b) kf_map_sample_device at 2^20 points within one voxel of the surface: vertices of the map mesh (kf_marching_cubes_map), jittered;
  (c) kf_map_cast_rays_device with the 640 x 480 camera rays of the tracked pose, beside kf_render_view_at of the current window for the same camera --
      the only way there was to get ray hits from the map; both are reported, nothing is asserted on the ratio (the view call shades an image too and
      walks skip tables the query does not have);
  (d) the same rays from half a window further back along the viewing axis: they cross empty space (bricks nobody holds: no loads), then store and window.
One JSON line per leg, also collected into the output file.  usage: tools/bench_map_query.py [c2|c4] [reps] [output file, default profiles/map_query_<cfg>.json]
HIP events on the context's stream around each leg, one warm-up, then the median of `reps` >= 5 (default 7).  The outputs of (a) and (b) are checked against
the host form of the same call once, before the timing."""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "map_query_%s.json" % cfg)
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
P = S.STOCK
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
med = statistics.median
nb = res // 8
f32 = np.float32
N = 1 << 20
common = dict(tool="bench_map_query", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []

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
pipe.ctx.raycast(None, pipe.inc, P["depth_trunc_min"], pipe.trunc_max)
held = ctx.brick_store_count()[0]
lo_b, hi_b = ctx.brick_store_bounds()
origin = np.array(ctx.volume_origin(), np.float64)
cell = f32(size) / f32(res)
rng = np.random.default_rng(7)
gpu = torch.device("cuda")

# the point sets
lo_v, hi_v = np.minimum(np.array(lo_b) * 8.0, origin), np.maximum(np.array(hi_b) * 8.0, origin + res)
pts_a = rng.uniform(lo_v, hi_v, (N, 3))
ctx.clear_triangles()
ctx.marching_cubes_map(300 * size / res)
tris = ctx.triangles()
verts = tris["v"]["pos"].reshape(-1, 3).astype(np.float64) / float(cell)        # world metres -> world voxels
assert len(verts) > 0
pts_b = verts[rng.integers(0, len(verts), N)] + rng.uniform(-1, 1, (N, 3))
ctx.clear_triangles()

d_pos = {"a": torch.from_numpy(pts_a).to(gpu), "b": torch.from_numpy(pts_b).to(gpu)}
o_t, o_w = torch.zeros(N, device=gpu), torch.zeros(N, device=gpu)
o_g, o_c = torch.zeros((N, 3), device=gpu), torch.zeros((N, 4), dtype=torch.uint8, device=gpu)
torch.cuda.synchronize()


def sample(which):
    ctx.map_sample_device(N, d_pos[which].data_ptr(), o_t.data_ptr(), o_w.data_ptr(), o_g.data_ptr(), o_c.data_ptr())


observed = {}
for which, pts in (("a", pts_a), ("b", pts_b)):
    sample(which)
    ctx.sync()
    host = ctx.map_sample(pts[:65536], want=("tsdf", "weight"))
    assert np.array_equal(o_t.cpu().numpy()[:65536].view(np.uint32), host["tsdf"].view(np.uint32)), "device and host form disagree"
    observed[which] = int(torch.count_nonzero(o_w).item())

# the ray sets: the tracked pose's camera rays, in world voxels
pose = ctx.track_result()[1].astype(np.float64)
cols, rows, cx, cy, fx, fy = cam
v, u = np.mgrid[0:rows, 0:cols]
local = np.stack([(u.reshape(-1) - cx) / fx, (v.reshape(-1) - cy) / fy, np.ones(cols * rows)], axis=1)
local /= np.linalg.norm(local, axis=1, keepdims=True)
dirs = np.ascontiguousarray((local @ pose[:3, :3].T).astype(f32))
n_rays = len(dirs)
cam_pos = pose[:3, 3] / float(cell) + origin
near, far = float(f32(P["depth_trunc_min"]) / cell), float(f32(pipe.trunc_max) / cell)
step = float(f32(pipe.inc) / cell)
back = pose[:3, 2] * (res / 2.0)                                  # (d): the camera half a window further back along its viewing axis
rays = {}
for name, o, t1 in (("c", cam_pos, far), ("d", cam_pos - back, far + res / 2.0)):
    rays[name] = (torch.from_numpy(np.broadcast_to(o, (n_rays, 3)).copy()).to(gpu), torch.from_numpy(dirs).to(gpu),
                  torch.full((n_rays,), near, device=gpu), torch.full((n_rays,), t1, device=gpu))
r_s = torch.zeros(n_rays, dtype=torch.uint8, device=gpu)
r_t, r_w = torch.zeros(n_rays, device=gpu), torch.zeros(n_rays, device=gpu)
r_n, r_c = torch.zeros((n_rays, 3), device=gpu), torch.zeros((n_rays, 4), dtype=torch.uint8, device=gpu)
torch.cuda.synchronize()


def cast(name):
    o, d, t0, t1 = rays[name]
    ctx.map_cast_rays_device(n_rays, o.data_ptr(), d.data_ptr(), t0.data_ptr(), t1.data_ptr(), step, 1 << 24, r_s.data_ptr(), r_t.data_ptr(), r_n.data_ptr(),
                             r_c.data_ptr(), r_w.data_ptr())


def view_at():
    ctx.render_view_at(K.VIEW_SHADED, ctx.volume_origin(), None, K.camera(*cam), pipe.inc, P["depth_trunc_min"], pipe.trunc_max)


hits = {}
for name in ("c", "d"):
    cast(name)
    ctx.sync()
    st = r_s.cpu().numpy()
    hits[name] = [int(np.count_nonzero(st == k)) for k in (K.RAY_MISS, K.RAY_HIT, K.RAY_BROKEN)]

line("scene", bricks_held=int(held), window_origin=[int(x) for x in origin], store_bounds_bricks=[list(lo_b), list(hi_b)], mesh_vertices=int(len(verts)),
     step_voxels=round(step, 4), near_far_voxels=[round(near, 2), round(far, 2)])
a = line("a_sample_random_points", timed(lambda: sample("a")), points=N, observed=observed["a"])
b = line("b_sample_points_at_the_surface", timed(lambda: sample("b")), points=N, observed=observed["b"])
c = line("c_cast_camera_rays", timed(lambda: cast("c")), rays=n_rays, miss_hit_broken=hits["c"])
cv = line("c_render_view_at_same_camera", timed(view_at), pixels=n_rays)
d = line("d_cast_rays_across_store_and_window", timed(lambda: cast("d")), rays=n_rays, miss_hit_broken=hits["d"])
line("ratios", ns_per_point_a=round(1e6 * a["ms"] / N, 3), ns_per_point_b=round(1e6 * b["ms"] / N, 3), cast_over_view_at=round(c["ms"] / cv["ms"], 4),
     d_over_c=round(d["ms"] / c["ms"], 4))
line("not_run", what="configurations other than the one named above; a colour context; the host forms' copies; no threshold is set on any leg")
with open(out_path, "w") as f:
    for d_ in lines:
        f.write(json.dumps(d_) + "\n")
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
