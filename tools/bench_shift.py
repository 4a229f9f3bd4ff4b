#!/usr/bin/env python3
"""The moving volume alone: after 150 fused frames of Scene S, time kf_shift_volume against the recipe a caller had before it
(kf_download_volume_device -> roll / zero in torch -> kf_upload_volume_device) and against a plain device-to-device copy of the
volume's bytes, then a 300-frame run with a shift + re-raycast every 100th frame against the same run without shifts.
One JSON line per leg.  usage: tools/bench_shift.py [c2|c4] [reps]
Legs (a) - (c): HIP events on the context's stream, one warm-up, then the median of `reps` >= 5.  Between two timed shifts by d the
volume is shifted back by -d (untimed), so every repetition moves about the same contents."""
import ctypes as C, json, os, statistics, sys, time
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
SHIFTS = [(8, 0, 0), (0, 8, 0), (0, 0, 8), (64, -64, 64)]
common = dict(tool="bench_shift", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)


def new_pipe():
    return SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device())


def run(pipe, first, count, shift_every=0):
    for k in range(first, first + count):
        pipe.process_frame_device(ptr(k), k, ptr(k + 1))
        if shift_every and (k + 1) % shift_every == 0:
            sgn = 1 if ((k + 1) // shift_every) % 2 else -1        # there and back: the model stays inside the window
            pipe.shift_volume(8 * sgn, 0, 0)


pipe = new_pipe()
ctx = pipe.ctx
run(pipe, 0, 150)
pipe.sync()
assert pipe.stats()["frames_lost"] == 0
stream = torch.cuda.ExternalStream(ctx.stream)
n_vox = res ** 3
vol_bytes = n_vox * 8


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, undo):
    fn(); undo(); ctx.sync()                                      # warm-up
    out = []
    for _ in range(reps):
        out.append(event_ms(fn)); undo(); ctx.sync()
    return out


# (b)'s scratch: two volume-sized planes and their rolled copies -- what the recipe costs in memory, too
t_in, w_in = torch.empty((res, res, res), dtype=torch.float32, device="cuda"), torch.empty((res, res, res), dtype=torch.float32, device="cuda")


def recipe(d):
    def slc(s):
        return slice(max(0, -s), res - max(0, s)), slice(max(0, s), res - max(0, -s))
    with torch.cuda.stream(stream):
        ctx.download_volume_device(0, res, t_in.data_ptr(), w_in.data_ptr())
        t_out, w_out = torch.zeros_like(t_in), torch.zeros_like(w_in)
        (zd, zs), (yd, ys), (xd, xs) = slc(d[2]), slc(d[1]), slc(d[0])
        t_out[zd, yd, xd] = t_in[zs, ys, xs]
        w_out[zd, yd, xd] = w_in[zs, ys, xs]
        ctx.upload_volume_device(0, res, t_out.data_ptr(), w_out.data_ptr())
        t_out.record_stream(stream); w_out.record_stream(stream)


worst = 0.0
for d in SHIFTS:
    back = tuple(-x for x in d)
    a = timed(lambda: ctx.shift_volume(*d), lambda: ctx.shift_volume(*back))
    b = timed(lambda: recipe(d), lambda: recipe(back))
    worst = max(worst, med(a) / med(b))
    print(json.dumps(dict(common, leg="a_vs_b", shift=list(d), shift_ms=round(med(a), 4), shift_ms_all=[round(x, 4) for x in a],
                          recipe_ms=round(med(b), 4), recipe_ms_all=[round(x, 4) for x in b], shift_over_recipe=round(med(a) / med(b), 4),
                          launches=res // 8, bytes_moved=2 * vol_bytes, shift_gbs=round(2 * vol_bytes / (med(a) * 1e-3) / 1e9, 1))), flush=True)
del t_in, w_in

# (c) the copy yardstick: one hipMemcpyAsync of the volume's bytes, device to device
hip = C.CDLL("libamdhip64.so")
src, dst = torch.empty(vol_bytes, dtype=torch.uint8, device="cuda"), torch.empty(vol_bytes, dtype=torch.uint8, device="cuda")
src.zero_(); torch.cuda.synchronize()


def copy():
    st = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(vol_bytes), 3, C.c_void_p(ctx.stream))
    assert st == 0, st


c = timed(copy, lambda: None)
print(json.dumps(dict(common, leg="c_copy", copy_ms=round(med(c), 4), copy_ms_all=[round(x, 4) for x in c], bytes_moved=2 * vol_bytes,
                      copy_gbs=round(2 * vol_bytes / (med(c) * 1e-3) / 1e9, 1))), flush=True)
del src, dst
pipe.close()


# (d) frames/s over 300 frames with a shift + re-raycast every 100th frame, against the same run without
def fps(shift_every):
    p = new_pipe()
    run(p, 0, 20); p.sync()
    t0 = time.perf_counter()
    run(p, 20, 300, shift_every)
    p.sync()
    dt = time.perf_counter() - t0
    lost = p.stats()["frames_lost"]
    org = p.volume_origin()
    p.close()
    return 300 / dt, lost, org


plain = [fps(0) for _ in range(3)]
moved = [fps(100) for _ in range(3)]
print(json.dumps(dict(common, leg="d_stream", frames=300, shift_every=100, fps_plain=round(med(x[0] for x in plain), 1),
                      fps_with_shifts=round(med(x[0] for x in moved), 1), fps_plain_all=[round(x[0], 1) for x in plain],
                      fps_with_shifts_all=[round(x[0], 1) for x in moved], frames_lost=[int(plain[0][1]), int(moved[0][1])],
                      origin_after=list(moved[0][2]))), flush=True)
sys.exit(0 if worst <= 1.0 else 1)
