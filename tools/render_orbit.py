#!/usr/bin/env python3
"""Pictures of a scanned model from an orbit of viewpoints: fuse Scene S, then render N poses on a circle around the volume's centre with
kf_render_view at a chosen size and mode, and write one picture per pose into a directory.
  usage: tools/render_orbit.py OUT_DIR [--n 12] [--size 640x480] [--mode normals|shaded|color] [--res 256] [--volume 3.0] [--frames 12] [--slabs N]
                               [--frame X Y Z | --world]
--slabs N: the same orbit through a LOCAL slab group of N members (kf_group_render_view: every member marches its own layers, the merge gives
the whole volume's picture -- the same bytes).
--frame X Y Z: the orbit of a window that stands at that origin (voxels of the first cube, multiples of 8) instead of the current one, with
kf_render_view_at: nothing moves; the poses are that frame's.
--world: an orbit of the MAP.  A brick store is reserved, the window is shifted half its width along x after the scan -- so half of what was scanned lives
in the store alone -- and every pose of the orbit around the FIRST cube's centre, given in world coordinates, is rendered in the frame hkf_view_frame
centres on its focus (what HybKinectfu::renderMapView does).
PNG through PIL where it is installed, binary PPM otherwise (no hit: black)."""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from hybkinectfu_amd import lib as K, scene as S
from hybkinectfu_amd import group as G, pipeline as PL

ap = argparse.ArgumentParser()
ap.add_argument("out_dir")
ap.add_argument("--n", type=int, default=12)
ap.add_argument("--size", default="640x480")
ap.add_argument("--mode", default="shaded", choices=("normals", "shaded", "color"))
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--volume", type=float, default=3.0)
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--slabs", type=int, default=0, help="render through a LOCAL slab group of N members")
ap.add_argument("--frame", type=int, nargs=3, metavar=("X", "Y", "Z"), help="render the window as it would stand at this origin (kf_render_view_at)")
ap.add_argument("--world", action="store_true", help="an orbit of the map: brick store, window shifted away, poses in world coordinates")
args = ap.parse_args()
if args.slabs and (args.frame or args.world):
    ap.error("--frame / --world: the brick store and kf_render_view_at are single-GPU features")
if args.frame and args.world:
    ap.error("--frame or --world, not both")
cols, rows = (int(v) for v in args.size.lower().split("x"))
mode = dict(normals=K.VIEW_NORMALS, shaded=K.VIEW_SHADED, color=K.VIEW_COLOR)[args.mode]
P, cam, size, res = S.STOCK, S.vga_camera(), args.volume, args.res
trunc = max(P["integrate_sdf_trunc"], 5 * size / res)
color = mode == K.VIEW_COLOR


def ramp(mm):                                                   # a picture to fuse: the depth as a colour ramp
    g = (mm // 8 % 256).astype(np.uint8)
    return np.stack([g, 255 - g, (g // 2 + 64).astype(np.uint8)], axis=-1)


group = ctx = None
if args.slabs:
    # the group tracks its frames itself (the same trajectory, from HybKinectfu::init's pose)
    params = G.stock_params()
    params.integrate = K.IntegrateParams(trunc, P["integrate_depth_trunc"])
    params.raycast = K.RaycastParams(P["raycast_increment_factor"] * trunc)
    group = G.Group.local(K.camera(*cam), res, size, [0] + [r[1] for r in PL.slab_ranges(res, args.slabs)], params=params, has_color=color)
    group.set_pose(S.pose0(size))
    for k in range(args.frames):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        group.frame(mm, k, rgb=ramp(mm) if color else None)
    group.sync()
else:
    ctx = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3, has_color=color)
    if args.world:
        ctx.brick_store_reserve((res // 8) ** 3)
    for k in range(args.frames):
        pose = S.trajectory_pose(k, size).astype(np.float32)
        mm = S.render_depth_mm(pose, cam, size)
        ctx.upload_depth_mm(mm)
        if color:
            ctx.upload_rgb(ramp(mm))
        ctx.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
        ctx.integrate(pose, trunc, P["integrate_depth_trunc"], has_color=color, angle_weight=color)
    if args.world:
        ctx.shift_volume(8 * (res // 16), 0, 0)
        print("window at", ctx.volume_origin(), " bricks in the store:", ctx.brick_store_count()[0])


def look(eye, target):
    """camera -> world: z towards the target, y down the image (world +y), float32"""
    z = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = x, np.cross(z, x), z, eye
    return p.astype(np.float32)


def save(path, bgra):
    rgb = np.ascontiguousarray(bgra[..., 2::-1]) * (bgra[..., 3:4] > 0)
    try:
        from PIL import Image
        Image.fromarray(rgb, "RGB").save(path + ".png")
        return path + ".png"
    except ImportError:
        with open(path + ".ppm", "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
            f.write(rgb.tobytes())
        return path + ".ppm"


os.makedirs(args.out_dir, exist_ok=True)
view_cam = K.camera(cols, rows, (cols - 1) / 2.0, (rows - 1) / 2.0, 525.0 * cols / 640.0, 525.0 * cols / 640.0)
centre = np.array([0.5 * size, 0.5 * size, 0.5 * size])
# the orbit starts at the scanning camera's side (-z) and swings a third of a turn to either side of it: what the scan saw and where it ends
for i in range(args.n):
    a = math.radians(-60.0 + 120.0 * i / max(args.n - 1, 1))
    eye = centre + 0.75 * size * np.array([math.sin(a), -0.15, -math.cos(a)])
    if group:
        group.render_view(mode, look(eye, centre), view_cam, 0.05, 4.0 * size)
        img = group.read_view()
    elif args.world:
        from hybkinectfu_amd import host_app as H
        frame, local = H.view_frame(look(eye, centre), size, res)
        ctx.render_view_at(mode, frame, local, view_cam, P["raycast_increment_factor"] * trunc, 0.05, 4.0 * size)
        img = ctx.read_view()
    elif args.frame:
        ctx.render_view_at(mode, args.frame, look(eye, centre), view_cam, P["raycast_increment_factor"] * trunc, 0.05, 4.0 * size)
        img = ctx.read_view()
    else:
        ctx.render_view(mode, look(eye, centre), view_cam, P["raycast_increment_factor"] * trunc, 0.05, 4.0 * size)
        img = ctx.read_view()
    print("%s  hits %d" % (save(os.path.join(args.out_dir, "orbit_%03d" % i), img), int((img[..., 3] == 255).sum())))
(group or ctx).close()
