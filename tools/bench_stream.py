#!/usr/bin/env python3
"""Streaming the departing surface: what it costs.  After the stock stream (150 fused frames of Scene S) it times, with HIP events on the context's
stream, one warm-up and then the median of `reps` >= 5 repetitions:
  (a) kf_marching_cubes over the whole volume -- the only way to get a strip's triangles before kf_marching_cubes_region;
  (b) kf_marching_cubes_region of a one-brick strip on each axis (the brick layer through the volume's centre), with kf_region_work's figures;
  (c) kf_shift_volume by one brick with and without stream-out, the window moved first so that the layer that leaves holds surface (asserted);
  (d) frames/s of 900 frames with a shift + re-raycast every 25th frame (there and back), with and without stream-out into a world soup, the
      window moved first so that every second shift streams a cap of the central sphere (asserted); five runs each, alternated.
One JSON line per leg, also written to profiles/stream_<config>.json.  usage: tools/bench_stream.py [c2|c4] [reps]"""
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
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
med = statistics.median
MAX_TRI, SOUP = 6500000, 2000000
thr = 300 * size / res
common = dict(tool="bench_stream", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []


def emit(**kw):
    line = json.dumps(dict(common, **kw))
    lines.append(line)
    print(line, flush=True)


def new_pipe():
    return SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device(), max_triangles=MAX_TRI)


def run(pipe, first, count, shift_every=0):
    for k in range(first, first + count):
        pipe.process_frame_device(ptr(k), k, ptr(k + 1))
        if shift_every and (k + 1) % shift_every == 0:
            sgn = 1 if ((k + 1) // shift_every) % 2 else -1
            pipe.shift_volume(8 * sgn, 0, 0)


pipe = new_pipe()
ctx = pipe.ctx
run(pipe, 0, 150)
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, undo):
    fn(); undo(); ctx.sync()
    out = []
    for _ in range(reps):
        out.append(event_ms(fn)); undo(); ctx.sync()
    return out


r4 = lambda xs: [round(x, 4) for x in xs]
whole = timed(lambda: ctx.marching_cubes(thr), ctx.clear_triangles)
ctx.marching_cubes(thr)
n_whole = len(ctx.triangles()); ctx.clear_triangles()
emit(leg="a_whole", whole_ms=round(med(whole), 4), whole_ms_all=r4(whole), triangles=n_whole)
b0 = (res // 16) * 8                                                # the brick layer through the centre
for axis in range(3):
    lo, hi = [0, 0, 0], [res, res, res]
    lo[axis], hi[axis] = b0, b0 + 8
    t = timed(lambda: ctx.marching_cubes_region(thr, lo, hi), ctx.clear_triangles)
    ctx.marching_cubes_region(thr, lo, hi)
    bricks, blocks = ctx.region_work()
    n = len(ctx.triangles()); ctx.clear_triangles()
    emit(leg="b_strip", axis="xyz"[axis], cells=[lo, hi], strip_ms=round(med(t), 4), strip_ms_all=r4(t), triangles=n, bricks_read=bricks, blocks_listed=blocks,
         bricks_total=(res // 8) ** 3, strip_over_whole=round(med(t) / med(whole), 4))
# (c) Scene S fills [0.25, 0.75] of the cube (and the stock integration distance stops short of its back wall), so the outermost brick layer holds no surface.  Each
# sample first moves the window (untimed, stream-out off) until the central sphere reaches into the layer that the timed one-brick shift pushes out.  That layer comes back empty, so every sample runs on a
# freshly fused window: both variants move the same contents.  The variants alternate.
pipe.close()


def fused_window(pre):
    global stream
    p = new_pipe()
    run(p, 0, 150); p.sync()
    stream = torch.cuda.ExternalStream(p.ctx.stream)
    p.ctx.world_soup_reserve(SOUP)
    p.ctx.shift_volume(*pre)
    return p


q = (int(0.36 * res) // 8) * 8                                    # the central sphere (radius 0.15 res) then begins 5 voxels outside the window: the layer that leaves cuts a cap off it
for d, pre in (((8, 0, 0), (q, 0, 0)), ((0, 8, 0), (0, q, 0)), ((0, 0, 8), (0, 0, q))):
    samples = {"plain": [], "stream": []}
    n_streamed = None
    for i, variant in enumerate(["stream", "plain"] + ["plain", "stream"] * reps):       # the first two: warm-up
        p = fused_window(pre)
        p.ctx.set_stream_out(variant == "stream", thr)
        p.ctx.sync()
        ms = event_ms(lambda: p.ctx.shift_volume(*d))
        if variant == "stream":
            n = p.ctx.world_soup_count()[0]
            assert n > 0, (d, "the departing layer holds no surface: this leg would time an empty extraction")
            assert n_streamed in (None, n)
            n_streamed = n
        if i >= 2:
            samples[variant].append(ms)
        p.close()
    a, b = samples["plain"], samples["stream"]
    emit(leg="c_shift", shift=list(d), window_moved_first=list(pre), shift_ms=round(med(a), 4), shift_ms_all=r4(a), shift_stream_ms=round(med(b), 4),
         shift_stream_ms_all=r4(b), triangles_streamed=n_streamed, stream_out_ms=round(med(b) - med(a), 4))

# (d) the stream: the window is moved along x after 20 frames so that the central sphere reaches the face; then 900 frames with a shift + re-raycast every 25th
# frame, there and back (every second one pushes out a layer that holds a cap of the sphere, which the frames in between fuse again).  The variants alternate.
N_TIMED = 900


def fps(stream_out):
    p = new_pipe()
    p.ctx.world_soup_reserve(SOUP)
    run(p, 0, 20)
    p.shift_volume(q, 0, 0)
    run(p, 20, 30); p.sync()
    p.ctx.set_stream_out(bool(stream_out), thr)
    t0 = time.perf_counter()
    run(p, 50, N_TIMED, 25)
    p.sync()
    dt = time.perf_counter() - t0
    lost, n = p.stats()["frames_lost"], p.ctx.world_soup_count()
    p.close()
    return N_TIMED / dt, int(lost), n


fps(True)                                                          # warm-up of both code paths
plain, moved = [], []
for _ in range(5):
    plain.append(fps(False)); moved.append(fps(True))
assert moved[0][2][0] > 0, "nothing was streamed"
emit(leg="d_stream", frames=N_TIMED, shift_every=25, runs="5 + 5, alternated", fps_shifts=round(med(x[0] for x in plain), 1), fps_shifts_all=[round(x[0], 1) for x in plain],
     fps_shifts_streamed=round(med(x[0] for x in moved), 1), fps_shifts_streamed_all=[round(x[0], 1) for x in moved],
     frames_lost=[plain[0][1], moved[0][1]], soup_triangles=moved[0][2][0], soup_dropped=moved[0][2][1])
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
open(os.path.join(ROOT, "profiles", "stream_%s.json" % cfg), "w").write("\n".join(lines) + "\n")
