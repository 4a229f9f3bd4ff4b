#!/usr/bin/env python3
"""The weld alone: fuse C2's usual frames of Scene S, extract, then weld the soup on the host (the weld saveMesh has always run:
soup read-back + host_app.mesh_from_soup) and on the device (kf_weld_mesh + kf_read_mesh), check that the two meshes are the
same bits, and print one JSON line.  usage: tools/bench_weld.py [c2|c4] [reps]
Device weld: events on the context's stream around kf_weld_mesh (the call blocks on a 4-byte read-back per round, which the
interval includes), the first call (it allocates the scratch) reported apart, then the median of `reps` warm calls."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hybkinectfu_amd import lib as K, host_app as H, scene as S
import bench

cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
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


def wall_ms(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter(); r = fn(); out.append((time.perf_counter() - t0) * 1e3)
    return r, out


# host side: what saveMesh does today
soup, t_soup = wall_ms(ctx.triangles, 3)
host, t_host = wall_ms(lambda: H.mesh_from_soup(soup, False), 3)

# device side
stream = torch.cuda.ExternalStream(ctx.stream)


def weld_event_ms():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream); ctx.weld_mesh(False, 1e-4); e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


first_ev, first_wall = weld_event_ms()
warm = [weld_event_ms() for _ in range(reps)]
mesh, t_read = wall_ms(lambda: ctx.read_mesh(False), 5)
nv, nf, rounds = ctx.mesh_counts()
same = all(np.array_equal(mesh[k].view(np.uint32), host[k].view(np.uint32)) for k in ("vertices", "normals", "faces"))
med = statistics.median
dev_ms, dev_wall = med(w[0] for w in warm), med(w[1] for w in warm)
line = dict(tool="bench_weld", config=cfg.upper(), resolution=res, size_m=size, device=torch.cuda.get_device_name(0),
            triangles=int(len(soup)), vertices=int(nv), faces=int(nf), rounds=int(rounds), same_bits_as_host_weld=bool(same),
            soup_readback_ms=round(med(t_soup), 3), host_weld_ms=round(med(t_host), 3),
            device_weld_first_call_ms=round(first_ev, 3), device_weld_ms=round(dev_ms, 3), device_weld_wall_ms=round(dev_wall, 3),
            device_weld_reps=reps, mesh_readback_ms=round(med(t_read), 3),
            host_path_ms=round(med(t_soup) + med(t_host), 3), device_path_ms=round(dev_ms + med(t_read), 3),
            speedup=round((med(t_soup) + med(t_host)) / (dev_ms + med(t_read)), 2))
print(json.dumps(line))
ctx.close()
sys.exit(0 if same else 1)
