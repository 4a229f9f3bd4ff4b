#!/usr/bin/env python3
"""The moving volume over a slab group: time kf_group_shift_volume at C4's 8-way geometry (1024^3 @ 6 m, a slab every 128 layers, halo 8) on one GPU
(LOCAL backend) against the only way a group could move its window before it -- per member kf_download_volume_device of the stored planes, a roll
in torch that takes the layers a member does not store from their owner's planes, kf_upload_volume_device: the recipe tools/bench_shift.py times
for one context.  Three legs: a one-brick z shift, a one-brick x shift, a z shift of a whole slab (128 layers).  HIP events on the group's
stream, one warm-up, then the median of 7; between two timed shifts by d the window is shifted back by -d (untimed).  One JSON line per leg, with the
bytes the plan feeds each member; --out FILE also appends them there (profiles/group_shift_c4.json).  No threshold: a measurement, not a gate.

usage: tools/bench_group_shift.py [--small] [--reps N] [--out FILE] [--rccl]
--small: 192^3 @ 3 m, 8 slabs of 24 layers -- a quick check of the tool itself.
--rccl (two or more devices): the same legs through RCCL_ALL, one member per device, even slabs; wall clock around enqueue + synchronise, the
recipe not repeated."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hybkinectfu_amd import group as G, lib as K, pipeline as PL, scene as S

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default="")
ap.add_argument("--rccl", action="store_true")
args = ap.parse_args()
res, size, gate = (192, 3.0, None) if args.small else (1024, 6.0, 6.0)
members, halo = 8, 8
slab = res // members
cam = S.vga_camera()
kcam = K.camera(*cam)
params = G.stock_params(trunc_max=gate, integ_dist=gate)
med = statistics.median
LEGS = [("z_one_brick", (0, 0, 8)), ("x_one_brick", (8, 0, 0)), ("z_whole_slab", (0, 0, slab))]
common = dict(tool="bench_group_shift", resolution=res, size_m=size, members=members, halo=halo, device=torch.cuda.get_device_name(0), reps=args.reps)


def emit(**kw):
    line = json.dumps(dict(common, **kw))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def fuse(g, n=3):
    for k in range(n):
        mm = torch.from_numpy(S.render_depth_mm(S.trajectory_pose(k, size), cam, size).astype(np.int16)).cuda()
        if g.n > 1 and len(set(devs)) > 1:
            per = [mm.to(torch.device("cuda", d)) for d in devs]
            g.frame_members([t.data_ptr() for t in per], k)
        else:
            g.frame(mm.data_ptr(), k)
        assert g.track_result()[0], k
        g.sync()


def fed_bytes(g, cuts, dz):
    per = [0] * (len(cuts) - 1)
    lb = g.members()[0].slab_layer_bytes()
    for _, to, b0, b1 in G.shift_plan(res, cuts, g.halo, dz):
        per[to] += (b1 - b0) * lb
    return per


# ---- LOCAL: native against the recipe, HIP events ---------------------------------------------------------------------------------------------------
devs = [0] * members
cuts = list(range(0, res + 1, slab))
g = G.Group.local(kcam, res, size, cuts, halo=halo, params=params)
fuse(g)
stream = torch.cuda.ExternalStream(g.stream(0))
ms = g.members()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, undo):
    fn(); undo(); g.sync()                                        # warm-up (the group's feed buffers grow here)
    out = []
    for _ in range(args.reps):
        out.append(event_ms(fn)); undo(); g.sync()
    return out


def recipe(d):
    """every member's stored planes out, rolled with the layers it does not store taken from their owner's planes, and back in"""
    dx, dy, dz = d

    def slc(s):
        return slice(max(0, -s), res - max(0, s)), slice(max(0, s), res - max(0, -s))
    (yd, ys), (xd, xs) = slc(dy), slc(dx)
    with torch.cuda.stream(stream):
        planes = []
        for m in ms:
            z0, z1 = m.stored
            t = torch.empty((z1 - z0, res, res), dtype=torch.float32, device="cuda")
            w = torch.empty_like(t)
            m.download_volume_device(z0, z1, t.data_ptr(), w.data_ptr())
            planes.append((t, w))
        for i, m in enumerate(ms):
            z0, z1 = m.stored
            t_out, w_out = torch.zeros_like(planes[i][0]), torch.zeros_like(planes[i][1])
            lo, hi = max(z0, -dz, 0), min(z1, res - dz)           # destination layers whose source lies in the volume
            z = lo
            while z < hi:
                q = z + dz
                if z0 <= q < z1:
                    j, s0, s1 = i, z0, z1                          # stored here
                else:
                    j = next(k for k in range(members) if cuts[k] <= q < cuts[k + 1])      # its owner
                    s0, s1 = cuts[j], cuts[j + 1]
                n = min(hi - z, s1 - q)
                t_out[z - z0:z - z0 + n, yd, xd] = planes[j][0][q - ms[j].stored[0]:q - ms[j].stored[0] + n, ys, xs]
                w_out[z - z0:z - z0 + n, yd, xd] = planes[j][1][q - ms[j].stored[0]:q - ms[j].stored[0] + n, ys, xs]
                z += n
            m.upload_volume_device(z0, z1, t_out.data_ptr(), w_out.data_ptr())
            t_out.record_stream(stream); w_out.record_stream(stream)
        for t, w in planes:
            t.record_stream(stream); w.record_stream(stream)


stored_bytes = sum((m.stored[1] - m.stored[0]) * res * res * 8 for m in ms)
for name, d in LEGS:
    back = tuple(-x for x in d)
    a = timed(lambda: g.shift_volume(*d), lambda: g.shift_volume(*back))
    b = timed(lambda: recipe(d), lambda: recipe(back))
    emit(backend="local", leg=name, shift=list(d), shift_ms=round(med(a), 4), shift_ms_all=[round(x, 4) for x in a], recipe_ms=round(med(b), 4),
         recipe_ms_all=[round(x, 4) for x in b], shift_over_recipe=round(med(a) / med(b), 4), stored_bytes=stored_bytes,
         fed_bytes_per_member=fed_bytes(g, cuts, d[2]), shift_gbs=round(2 * stored_bytes / (med(a) * 1e-3) / 1e9, 1))
g.close()
del ms, stream
torch.cuda.empty_cache()

# ---- RCCL_ALL over every visible device ---------------------------------------------------------------------------------------------------------------
if args.rccl:
    ndev = torch.cuda.device_count()
    if ndev < 2:
        sys.exit("--rccl needs two or more visible devices")
    devs = list(range(ndev))
    cuts = [0] + [r[1] for r in PL.slab_ranges(res, ndev)]
    g = G.Group.rccl_all(kcam, res, size, cuts, devices=devs, halo=halo, params=params)
    fuse(g)
    for name, d in [(n, (dd[0], dd[1], min(dd[2], cuts[1]))) for n, dd in LEGS]:
        back = tuple(-x for x in d)
        g.shift_volume(*d); g.shift_volume(*back); g.sync()
        out = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); g.shift_volume(*d); g.sync(); out.append(1e3 * (time.perf_counter() - t0))
            g.shift_volume(*back); g.sync()
        emit(backend="rccl_all", members=ndev, leg=name, shift=list(d), shift_wall_ms=round(med(out), 4), shift_wall_ms_all=[round(x, 4) for x in out],
             fed_bytes_per_member=fed_bytes(g, cuts, d[2]))
    g.close()
