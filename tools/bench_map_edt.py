#!/usr/bin/env python3
"""What the map's distance field costs: after 150 fused frames of Scene S, with a brick store reserved and the window shifted half its width along x and
captured (the map of tools/bench_map_query.py), kf_map_distance_field_device runs over boxes of the map, occupied voxels as sites, both outputs asked for.
  (a) a 256^3 box around the tracked pose at a radius of 32 voxels;
  (b) the same box at a radius of 128;
  (c) a 128^3 box in empty space (nobody holds a brick within its radius of 32: no voxel loads, every voxel walks the full window);
  (s) a 256^3 box around the middle of the first cube, where the scene's surfaces are, at a radius of 32: the box of (a) holds free space in front of the
      scene and no surface of its own, this one is cut by the walls and the spheres;
  (d) the time of each kernel of (a) -- classify, x pass, y pass, z pass -- from a kernel trace taken in a run of its own (rocprofv3 --kernel-trace -- this
      tool with --legs a) and named with --kernel-trace FILE (the trace's CSV); without that file the leg says "not measured";
  (e) the only way there was before: the store read out, the window downloaded, the dense box assembled on the host and scipy.ndimage's
      distance_transform_edt run on it (the numpy restatement of tests/map_edt_expect.py where scipy is absent), by host clock, once.  Its result is compared
      with (a)'s, which must agree voxel for voxel.
One JSON line per leg, also collected into the output file.
usage: tools/bench_map_edt.py [c2|c4] [reps] [output file, default profiles/map_edt_<cfg>.json] [--legs a] [--kernel-trace FILE]
HIP events on the context's stream around each leg, one warm-up, then the median of `reps` >= 5 (default 7).  No threshold is set on any figure."""
import csv, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from hybkinectfu_amd import lib as K, scene as S
from hybkinectfu_amd.pipeline import SingleGpuPipeline
import bench
import map_edt_expect as E

argv = list(sys.argv[1:])
only = argv.pop(argv.index("--legs") + 1) if "--legs" in argv else None
if "--legs" in argv:
    argv.remove("--legs")
ktrace = argv.pop(argv.index("--kernel-trace") + 1) if "--kernel-trace" in argv else None
if "--kernel-trace" in argv:
    argv.remove("--kernel-trace")
cfg = argv[0] if len(argv) > 0 else "c2"
reps = max(5, int(argv[1])) if len(argv) > 1 else 7
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "map_edt_%s.json" % cfg)
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
OCC = 1 << K.VOX_OCCUPIED
common = dict(tool="bench_map_edt", config=wl["name"], resolution=res, size_m=size, device=torch.cuda.get_device_name(0), reps=reps)
lines = []

pipe = SingleGpuPipeline(K.camera(*cam), res, size, wl, device=torch.cuda.current_device(), max_triangles=0)
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
        if rep:                                                   # (the first one is the warm-up; it also grows the scratch)
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
origin = np.array(ctx.volume_origin(), np.int64)
cell = f32(size) / f32(res)
pose = ctx.track_result()[1].astype(np.float64)
cam_vox = np.floor(pose[:3, 3] / float(cell)).astype(np.int64) + origin
gpu = torch.device("cuda")

BOX = 256
lo_a = tuple(int(v) - BOX // 2 for v in cam_vox)
lo_s = (res // 2 - BOX // 2,) * 3                                  # the scene's middle (Scene S is centred in the first cube)
lo_c = (8 * int(hi_b[0]) + 512, 8 * int(hi_b[1]) + 512, 8 * int(hi_b[2]) + 512)      # beyond everything the store and the window hold
o_d = torch.zeros(BOX ** 3, dtype=torch.int16, device=gpu)
o_c = torch.zeros(BOX ** 3, dtype=torch.uint8, device=gpu)
torch.cuda.synchronize()


def field(lo, n, radius):
    ctx.map_distance_field_device(lo, (n, n, n), radius, 0.0, OCC, o_d.data_ptr(), o_c.data_ptr())


def census(n):
    ctx.sync()
    d = o_d.cpu().numpy().view(np.uint16)[:n ** 3]
    c = o_c.cpu().numpy()[:n ** 3]
    return dict(within_radius=int(np.count_nonzero(d != K.EDT_FAR)), sites=int(np.count_nonzero(d == 0)), unknown_free_occupied=[int(np.count_nonzero(c == k)) for k in range(3)])


line("scene", bricks_held=int(held), window_origin=[int(x) for x in origin], store_bounds_bricks=[list(lo_b), list(hi_b)], box_a_lo=list(lo_a), box_c_lo=list(lo_c))
field(lo_a, BOX, 32)
cen_a = census(BOX)
got_a = o_d.cpu().numpy().view(np.uint16).reshape(BOX, BOX, BOX).copy()
a = line("a_box256_radius32", timed(lambda: field(lo_a, BOX, 32)), voxels=BOX ** 3, **cen_a)
if only != "a":
    field(lo_a, BOX, 128)
    cen_b = census(BOX)
    b = line("b_box256_radius128", timed(lambda: field(lo_a, BOX, 128)), voxels=BOX ** 3, **cen_b)
    field(lo_c, 128, 32)
    cen_c = census(128)
    c = line("c_box128_empty_radius32", timed(lambda: field(lo_c, 128, 32)), voxels=128 ** 3, **cen_c)

    field(lo_s, BOX, 32)
    cen_s = census(BOX)
    s_ = line("s_box256_at_the_scene_radius32", timed(lambda: field(lo_s, BOX, 32)), voxels=BOX ** 3, box_lo=list(lo_s), **cen_s)

    # (d) per kernel, from a trace of a run of its own
    if ktrace and os.path.exists(ktrace):
        # the trace's dispatches in start order: every call is classify, x pass, then k_edt_pass twice -- the y pass first, the z pass second
        rows = sorted((r for r in csv.DictReader(open(ktrace)) if "k_edt" in r.get("Kernel_Name", "")), key=lambda r: int(r["Start_Timestamp"]))
        per, n_pass = {}, 0
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            if name == "k_edt_pass":
                name, n_pass = ("k_edt_pass (y pass)", "k_edt_pass (z pass)")[n_pass % 2], n_pass + 1
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        line("d_per_kernel_of_a", source="rocprofv3 --kernel-trace, a run with --legs a (%d calls of the field, radius 32); the two k_edt_pass launches of a call told apart by their order" % (reps + 2),
             kernels=[dict(name=k, calls=len(v), median_us=round(med(v), 2), mean_us=round(sum(v) / len(v), 2)) for k, v in per.items()])
    else:
        line("d_per_kernel_of_a", not_measured="no kernel trace named: rocprofv3 --kernel-trace -- tools/bench_map_edt.py c2 7 OUT --legs a, then --kernel-trace FILE")

    # (e) the way there was before, on the host
    R = 32
    t0 = time.perf_counter()
    keys, t, w, _ = ctx.brick_store(color=False)
    t1 = time.perf_counter()
    vt, vw = ctx.download_volume()[:2]
    t2 = time.perf_counter()
    n = BOX + 2 * R
    lo_h = np.array(lo_a, np.int64) - R
    cls = np.zeros((n, n, n), np.uint8)

    def paste(k, bt, bw):
        o = 8 * np.asarray(k, np.int64) - lo_h
        p, q = np.maximum(o, 0), np.minimum(o + 8, n)
        if np.all(p < q):
            cl = E.np_classify(bt, bw, 0.0)
            cls[p[2]:q[2], p[1]:q[1], p[0]:q[0]] = cl[p[2] - o[2]:q[2] - o[2], p[1] - o[1]:q[1] - o[1], p[0] - o[0]:q[0] - o[0]]
    inside = np.all((keys * 8 >= lo_h - 7) & (keys * 8 < lo_h + n), axis=1)
    for i in np.flatnonzero(inside):
        paste(keys[i], t[i], w[i])
    wo = origin - lo_h                                            # the window over it: its copy wins
    p, q = np.maximum(wo, 0), np.minimum(wo + res, n)
    if np.all(p < q):
        part = (slice(p[2] - wo[2], q[2] - wo[2]), slice(p[1] - wo[1], q[1] - wo[1]), slice(p[0] - wo[0], q[0] - wo[0]))
        cls[p[2]:q[2], p[1]:q[1], p[0]:q[0]] = E.np_classify(vt[part], vw[part], 0.0)
    t3 = time.perf_counter()
    site = cls == E.OCCUPIED
    try:
        import scipy.ndimage as ndi
        how = "scipy.ndimage.distance_transform_edt"
        dd = ndi.distance_transform_edt(~site)[R:R + BOX, R:R + BOX, R:R + BOX] if site.any() else np.full((BOX, BOX, BOX), 1e9)
        d2 = np.rint(dd * dd)
        host = np.where(d2 <= R * R, d2, E.FAR).astype(np.uint16)
    except ImportError:
        how = "tests/map_edt_expect.py np_edt"
        host = E.np_edt(site, R, (BOX, BOX, BOX))
    t4 = time.perf_counter()
    same = bool(np.array_equal(host, got_a))
    e = line("e_host_readout_assembly_transform", how=how, ms=[1e3 * (t4 - t0)], read_store_ms=round(1e3 * (t1 - t0), 2), download_window_ms=round(1e3 * (t2 - t1), 2),
             assemble_ms=round(1e3 * (t3 - t2), 2), transform_ms=round(1e3 * (t4 - t3), 2), equals_a=same, differing_voxels=int(np.count_nonzero(host != got_a)))
    line("ratios", a_over_e=round(a["ms"] / e["ms"], 6), e_over_a=round(e["ms"] / a["ms"], 1), b_over_a=round(b["ms"] / a["ms"], 3), s_over_a=round(s_["ms"] / a["ms"], 3), ns_per_voxel_a=round(1e6 * a["ms"] / BOX ** 3, 4),
         ns_per_voxel_c=round(1e6 * c["ms"] / 128 ** 3, 4))
    line("not_run", what="configurations other than the one named above; a colour context; the host form's copies; a scan-based y / z pass (Meijster, Felzenszwalb): only the "
                         "windowed pass with the exact prune was built, so there is no second candidate's time to record; no threshold is set on any leg")
    with open(out_path, "w") as f:
        for d_ in lines:
            f.write(json.dumps(d_) + "\n")
ctx.brick_store_reserve(0)
ctx.sync()
pipe.close()
