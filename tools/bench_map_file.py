#!/usr/bin/env python3
"""What saving and loading the map costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x (as
in tools/bench_view_at.py: the surface in the half that left lives in the store alone),
  (a) kf_brick_store_capture: the window's observed bricks into the store;
  (b) the store read out in chunks (kf_read_brick_store) and written as a map file, each record at its place among the sorted keys, in HybKinectfu's chunk size;
  (c) the file read back and written into a fresh store (kf_write_brick_store), chunk by chunk;
  (d) kf_place_window at the saved origin: capture, clears, restore of all bricks;
  (e) the only way there was to carry a window across processes: a dense kf_download_volume + kf_upload_volume of the window -- which carries the
      window alone, not the map;
  (f) HybKinectfu::saveMap and (g) HybKinectfu::loadMap end to end on a model the host class fused from the same frames: the C++ codec, host clock.
In (b) and (c) the file codec is numpy's, in this tool; (f) and (g) time host/map_file.cpp.
One JSON line per leg.  usage: tools/bench_map_file.py [c2|c4] [reps] [directory for the file, default: the system's temporary directory]
HIP events on the context's stream around each leg (host work between the events included: the legs (b), (c) and (e) are host-bound), one warm-up, then
the median of `reps` >= 5 (default 7).  (c) + (d) are checked to reproduce the planes before they are timed."""
import json, os, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hybkinectfu_amd import lib as K, scene as S
from hybkinectfu_amd.pipeline import SingleGpuPipeline
import bench

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
out_dir = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
wl = bench.workload(1, cfg)
cam, res, size = wl["cam"], wl["res"], wl["size"]
N_UNIQUE = 100                                                    # the camera path has period 100
frames, _ = S.make_stream(N_UNIQUE, cam, size)
dev = torch.from_numpy(frames.astype(np.int16)).cuda()
fb = cam[0] * cam[1] * 2
ptr = lambda k: dev.data_ptr() + (k % N_UNIQUE) * fb
med = statistics.median
nb = res // 8
CHUNK = 256                                                       # HybKinectfu::saveMap / loadMap's chunk
common = dict(tool="bench_map_file", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)

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


def line(leg, ms, **kw):
    print(json.dumps(dict(common, leg=leg, ms=round(med(ms), 4), ms_all=[round(x, 4) for x in ms], **kw)), flush=True)


ctx.brick_store_reserve(nb ** 3)
d = (8 * (nb // 2), 0, 0)
ctx.shift_volume(*d)
here = ctx.volume_origin()
in_store = ctx.brick_store_count()[0]
path = os.path.join(out_dir, "bench_map_file.hkfmap")
REC = 12 + 2048 + 2048


def capture():
    ctx.brick_store_capture()


def save():
    """the store in chunks, each record at its place among the sorted keys: what hkf_map_write does, with numpy as the codec"""
    n = ctx.brick_store_count()[0]
    keys = np.zeros((n, 3), np.int32)
    for first in range(0, n, CHUNK):
        c = min(CHUNK, n - first)
        K._chk(ctx.lib.kf_read_brick_store(ctx.h, first, c, K._p(keys[first:first + c]), None, None, None), "kf_read_brick_store")
    rank = np.empty(n, np.int64)
    rank[np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))] = np.arange(n)
    t, w = np.zeros((CHUNK, 512), np.float32), np.zeros((CHUNK, 512), np.float32)
    with open(path, "wb") as f:
        f.write(b"\0" * 128)                                      # (the header's bytes do not matter to the timing)
        for first in range(0, n, CHUNK):
            c = min(CHUNK, n - first)
            K._chk(ctx.lib.kf_read_brick_store(ctx.h, first, c, None, K._p(t), K._p(w), None), "kf_read_brick_store")
            for i in range(c):
                f.seek(128 + REC * int(rank[first + i]))
                f.write(keys[first + i].tobytes()); f.write(t[i].tobytes()); f.write(w[i].tobytes())
    return n


def load():
    n = (os.path.getsize(path) - 128) // REC
    with open(path, "rb") as f:
        f.seek(128)
        for first in range(0, n, CHUNK):
            c = min(CHUNK, n - first)
            rec = np.frombuffer(f.read(REC * c), np.uint8).reshape(c, REC)
            keys = np.ascontiguousarray(rec[:, :12]).view(np.int32)
            t = np.ascontiguousarray(rec[:, 12:2060]).view(np.float32)
            w = np.ascontiguousarray(rec[:, 2060:]).view(np.float32)
            ctx.write_brick_store(keys, t, w)


def place():
    ctx.place_window(*here)


def dense():
    t, w = ctx.download_volume()
    ctx.upload_volume(t, w)


capture()
held = save()
planes = ctx.download_volume()
print(json.dumps(dict(common, leg="scene", bricks_total=nb ** 3, shift=list(d), bricks_in_store_before_capture=int(in_store), bricks_in_map=int(held),
                      file_bytes=os.path.getsize(path))), flush=True)
ctx.brick_store_clear(); load(); place()                         # the map from the file alone gives the window back
back = ctx.download_volume()
assert np.array_equal(planes[0].view(np.uint32), back[0].view(np.uint32)) and np.array_equal(planes[1].view(np.uint32), back[1].view(np.uint32))
line("a_capture", timed(capture), bricks=int(held))
line("b_read_out_and_write_file", timed(save), bricks=int(held), file_bytes=os.path.getsize(path))
line("c_read_file_and_write_store", timed(load, before=ctx.brick_store_clear), bricks=int(held))
line("d_place_window", timed(place), bricks=int(held))
line("e_dense_download_upload", timed(dense), window_bytes=int(planes[0].nbytes + planes[1].nbytes))
os.remove(path)
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()

# (f), (g): the host class end to end, with the C++ codec of host/map_file.cpp -- what a user of HybKinectfu pays.  A second model, fused by the host
# class from the same frames and shifted the same way; save_map and load_map are blocking calls, timed with the host clock around them.
import time
from hybkinectfu_amd import host_app as H


def host_ms(fn):
    out = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        assert fn()
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            out.append(ms)
    return out


app = H.App(res, size, cam, trunc_max=wl["trunc_max"], integrate_dist=wl["integ_dist"])
app.set_brick_store(nb ** 3)
for k in range(150):
    assert app.process_frame(frames[k % N_UNIQUE], k), k
assert app.shift_volume(*d)
f_ms = host_ms(lambda: app.save_map(path))
info = H.map_file_info(path)
line("f_app_save_map", f_ms, bricks=info["n_bricks"], file_bytes=os.path.getsize(path), clock="host", includes="capture, read-out in chunks of 256, the C++ codec's file write")
g_ms = host_ms(lambda: app.load_map(path))
line("g_app_load_map", g_ms, bricks=info["n_bricks"], clock="host", includes="whole-file check, reset, store reserve, the C++ codec's file read, kf_write_brick_store per chunk, kf_place_window, raycast")
assert app.brick_store_count()[0] == info["n_bricks"] and app.volume_origin() == info["origin_vox"]
app.close()
os.remove(path)
