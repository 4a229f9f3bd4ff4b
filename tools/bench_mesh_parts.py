#!/usr/bin/env python3
"""The parts of the mesh on C2's soup: fuse C2's usual frames of Scene S, extract, weld, then label the mesh's parts and drop the small ones on the
device (kf_mesh_parts, kf_mesh_drop_parts at min_faces 100) and on one host thread (mesh_parts.hpp's dropParts on the same mesh), check that both
give the same bytes, and print one JSON line per leg: (a) kf_weld_mesh, (b) kf_mesh_parts, (c) kf_mesh_drop_parts, (d) host dropParts, (e) the
labelling rounds of the 9000-triangle strips of tests/test_mesh_parts_cpu.py.  usage: tools/bench_mesh_parts.py [c2|c4] [reps]
Device legs: events on the context's stream around the call (each blocks on its 4-byte read-backs, which the interval includes); the first call
(it allocates) apart, then the median of `reps` warm calls, every one on a fresh weld."""
import ctypes as C
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from hybkinectfu_amd import lib as K, host_app as H, scene as S
import bench
import test_mesh_parts_cpu as R

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
MIN_FACES = 100
wl = bench.workload(1, cfg)
cam, P = wl["cam"], S.STOCK
res, size = wl["res"], wl["size"]
ctx = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3, max_triangles=8_000_000)
for k in range(0, 12, 3):
    pose = S.trajectory_pose(k, size).astype(np.float32)
    ctx.upload_depth_mm(S.render_depth_mm(pose, cam, size))
    ctx.preprocess(P["depth_trunc_min"], wl["trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
    ctx.integrate(pose, P["integrate_sdf_trunc"], wl["integ_dist"])
ctx.marching_cubes(300.0 * size / res)
ctx.sync()
soup = ctx.triangles()
stream = torch.cuda.ExternalStream(ctx.stream)
med = statistics.median
common = dict(tool="bench_mesh_parts", config=cfg.upper(), resolution=res, size_m=size, device=torch.cuda.get_device_name(0), triangles=int(len(soup)), reps=reps)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream); r = fn(); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def one_pass():
    """weld, label, drop: the three intervals and what the calls returned"""
    t_weld, _ = event_ms(lambda: ctx.weld_mesh(False, 1e-4))
    t_parts, parts = event_ms(ctx.mesh_parts)
    t_drop, dropped = event_ms(lambda: ctx.mesh_drop_parts(MIN_FACES, False))
    return t_weld, t_parts, t_drop, parts, dropped


first = one_pass()
warm = [one_pass() for _ in range(reps)]
ctx.weld_mesh(False, 1e-4)
nv, nf, _ = ctx.mesh_counts()
full = ctx.read_mesh()
ctx.mesh_drop_parts(MIN_FACES, False)
dev = ctx.read_mesh()
n_parts, largest, orphans, rounds = warm[-1][3]

# the host leg: dropParts alone, on the mesh the host weld makes of the same soup (the same bits as the device's)
h = H.load()
t_host = []
for _ in range(reps):
    H.mesh_from_soup(soup, False)
    t0 = time.perf_counter(); h.hkf_mesh_drop_parts(0, C.c_uint32(MIN_FACES), 0); t_host.append((time.perf_counter() - t0) * 1e3)
host = H._mesh_read(0)
want, pd, od = R.np_drop(full, MIN_FACES, False)
same = all(dev[k].tobytes() == host[k].tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in ("vertices", "normals", "faces"))

a, b, c = med(w[0] for w in warm), med(w[1] for w in warm), med(w[2] for w in warm)
print(json.dumps(dict(common, leg="a kf_weld_mesh", vertices=int(nv), faces=int(nf), first_call_ms=round(first[0], 3), ms=round(a, 3))))
print(json.dumps(dict(common, leg="b kf_mesh_parts", parts=int(n_parts), largest_faces=int(largest), orphans=int(orphans), n_rounds=int(rounds),
                      first_call_ms=round(first[1], 3), ms=round(b, 3))))
print(json.dumps(dict(common, leg="c kf_mesh_drop_parts", min_faces=MIN_FACES, parts_dropped=int(warm[-1][4][0]), orphans_dropped=int(warm[-1][4][1]),
                      vertices_left=int(len(dev["vertices"])), faces_left=int(len(dev["faces"])), first_call_ms=round(first[2], 3), ms=round(c, 3))))
print(json.dumps(dict(common, leg="d host dropParts, one thread", min_faces=MIN_FACES, ms=round(med(t_host), 3), same_bytes_device_host_numpy=bool(same),
                      device_parts_plus_drop_ms=round(b + c, 3), host_over_device=round(med(t_host) / (b + c), 2), device_over_weld=round((b + c) / a, 2))))
ctx.close()

small = K.Context(K.camera(160, 120, 79.5, 59.5, 131.25, 131.25), 32, 3.0, levels=3, max_triangles=10000)
strips = {}
for order in ("ascending", "descending", "permuted"):
    small.write_triangles(R.CASES["strip_" + order][0])
    small.weld_mesh(False, 1e-4)
    parts = small.mesh_parts()
    strips[order] = dict(parts=parts[0], n_rounds=parts[3])
small.close()
print(json.dumps(dict(common, leg="e strips of 9000 triangles", strips=strips)))
sys.exit(0 if same else 1)
