"""The volumes and viewpoints of tests/test_gpu_raycast_forms.py and tests/test_gpu_raycast_sides.py: what the raycast's child process
(raycast_forms_child.py) casts on the GPU and what the parent casts with the CPU oracle.

Every volume but one is analytic (numpy, deterministic) and is uploaded identically to the context (kf_upload_volume, which rebuilds the brick flags
and the macro / super / meso tables) and to the oracle's volume, so the raycast is tested apart from integrate.  The last one is fused from Scene S
on both sides from three directions, which checks the flags the fusion pass maintains.  The viewpoints look at the volumes from every side: falling
rays (dir.z < 0), every sign combination, from inside the volume and inside a solid, rolled, from far away, with near / far planes that cut surfaces,
grazing a face, with exactly zero direction components and from a macro-cell boundary plane."""
import math

import numpy as np

import oracle_lib as O
from hybkinectfu_amd import scene as S

P = S.STOCK
RAGGED = (200, 152, 99.5, 75.5, 164.0, 164.0)          # test_gpu_parity.ragged_cam: no multiple of the 32x16 ray tile
ODD = (101, 77, 50.0, 38.0, 82.0, 82.0)                # test_gpu_parity.odd_cam: integer cx, cy -- the centre column / row has a zero component
VGA = S.vga_camera()
NEAR, FAR = P["depth_trunc_min"], P["depth_trunc_max"]


# ---- analytic volumes ---------------------------------------------------------------------------------------------------------------------------
def _box(px, py, pz, lo, hi):
    qx, qy, qz = np.maximum(lo[0] - px, px - hi[0]), np.maximum(lo[1] - py, py - hi[1]), np.maximum(lo[2] - pz, pz - hi[2])
    out = np.sqrt(np.maximum(qx, 0) ** 2 + np.maximum(qy, 0) ** 2 + np.maximum(qz, 0) ** 2)
    return out + np.minimum(np.maximum(np.maximum(qx, qy), qz), 0)


def _sphere(px, py, pz, c, r):
    return np.sqrt((px - c[0]) ** 2 + (py - c[1]) ** 2 + (pz - c[2]) ** 2) - r


def analytic_sdf(px, py, pz, res):
    """signed distance (fractions of the volume's edge) of the solids, at points given as fractions of the edge"""
    # a hollow box shell (faces towards all six axis directions, outside and in) with a window through its two z walls, a sphere inside it
    shell = np.maximum(_box(px, py, pz, (0.30, 0.30, 0.30), (0.70, 0.70, 0.70)), -_box(px, py, pz, (0.34, 0.34, 0.34), (0.66, 0.66, 0.66)))
    shell = np.maximum(shell, -_box(px, py, pz, (0.44, 0.44, -1.0), (0.56, 0.56, 2.0)))
    d = np.minimum(shell, _sphere(px, py, pz, (0.5, 0.5, 0.5), 0.07))
    # free spheres; the first one holds a camera position (VIEWS "in-solid")
    d = np.minimum(d, _sphere(px, py, pz, (0.16, 0.20, 0.80), 0.09))
    d = np.minimum(d, _sphere(px, py, pz, (0.82, 0.16, 0.24), 0.07))
    # a slanted slab, clipped by a box
    n = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    plane = np.abs((px - 0.17) * n[0] + (py - 0.82) * n[1] + (pz - 0.30) * n[2]) - 0.025
    d = np.minimum(d, np.maximum(plane, _box(px, py, pz, (0.05, 0.70, 0.10), (0.30, 0.95, 0.50))))
    # a box through the +x face of the volume (the march and the gradient at the clamp), one within two voxels of the -y face
    d = np.minimum(d, _box(px, py, pz, (0.86, 0.60, 0.55), (1.30, 0.90, 0.85)))
    d = np.minimum(d, _box(px, py, pz, (0.50, 1.5 / res, 0.05), (0.72, 0.12, 0.20)))
    return d


def analytic_volume(res, size, color=False):
    """(tsdf, weight, rgb or None) as [z][y][x] arrays: tsdf = sdf / trunc clamped to [-1, 1], weight 2 wherever the sdf exceeds -trunc (seen free
    space and the band); deeper inside the solids tsdf 0, weight 0 (never observed, as after fusion).  trunc = 5 voxels."""
    trunc = 5.0 / res                                   # (fraction of the edge)
    tsdf = np.empty((res, res, res), np.float32)
    weight = np.empty((res, res, res), np.float32)
    c = (np.arange(res, dtype=np.float64) + 0.5) / res
    py, px = np.meshgrid(c, c, indexing="ij")
    for z in range(res):
        d = analytic_sdf(px, py, np.full_like(px, c[z]), res)
        seen = d > -trunc
        tsdf[z] = np.where(seen, np.clip(d / trunc, -1.0, 1.0), 0.0)
        weight[z] = np.where(seen, 2.0, 0.0)
    rgb = None
    if color:
        i = np.arange(res, dtype=np.int64)
        rgb = np.empty((res, res, res, 3), np.uint8)
        rgb[..., 0] = ((i[None, None, :] * 37 + i[:, None, None] * 5) % 256).astype(np.uint8)
        rgb[..., 1] = ((i[None, :, None] * 23 + 40) % 256).astype(np.uint8)
        rgb[..., 2] = ((i[:, None, None] * 11 + i[None, :, None] * 3 + 90) % 256).astype(np.uint8)
    return tsdf, weight, rgb


# ---- viewpoints -----------------------------------------------------------------------------------------------------------------------------------
def look(eye, fwd, up=(0.0, -1.0, 0.0), roll_deg=0.0):
    """camera -> world pose in float64 with an orthonormal rotation: camera z along fwd, camera y (image down) against `up`, rolled about z; cast to
    float32 by the caller"""
    z = np.asarray(fwd, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64) * -1.0, z)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross((1.0, 0.0, 0.0), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    r = math.radians(roll_deg)
    xr, yr = math.cos(r) * x + math.sin(r) * y, -math.sin(r) * x + math.cos(r) * y
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = xr, yr, z, eye
    return p


def axes(cols, eye):
    """a rotation with entries exactly 0 / +-1: `cols` = the world axes of camera x, y, z as signed axis numbers (1 = +x, -3 = -z)"""
    p = np.eye(4)
    for j, a in enumerate(cols):
        p[:3, j] = 0.0
        p[abs(a) - 1, j] = math.copysign(1.0, a)
    p[:3, 3] = eye
    return p


def views(size, res):
    """[(name, pose float64, near, far)]: the viewpoints at a volume of edge `size`"""
    s = size
    mp = [32 * round(res * f / 32) * (size / res) for f in (0.5, 0.5, 0.9)]
    v = [
        ("front+z", look((0.5 * s, 0.5 * s, -0.35 * s), (0, 0, 1)), NEAR, FAR),
        ("back-z", look((0.47 * s, 0.52 * s, 1.35 * s), (0.02, -0.01, -1)), NEAR, FAR),
        ("side+x", look((-0.4 * s, 0.45 * s, 0.55 * s), (1, 0.03, -0.02)), NEAR, FAR),
        ("side-x", look((1.4 * s, 0.55 * s, 0.45 * s), (-1, -0.02, 0.03)), NEAR, FAR),
        ("top+y", look((0.52 * s, -0.4 * s, 0.5 * s), (0.01, 1, 0.02), up=(0, 0, 1)), NEAR, FAR),
        ("bottom-y", look((0.48 * s, 1.4 * s, 0.5 * s), (-0.02, -1, 0.01), up=(0, 0, 1)), NEAR, FAR),
        ("corner-mixed", look((1.25 * s, -0.3 * s, 1.3 * s), (-0.75, 0.8, -0.8)), NEAR, 3.0 * s),
        ("corner-low", look((-0.3 * s, -0.25 * s, -0.35 * s), (0.8, 0.75, 0.85)), NEAR, 3.0 * s),
        ("inside+z", look((0.18 * s, 0.5 * s, 0.06 * s), (0.2, 0.05, 1)), 0.05, FAR),
        ("inside-z", look((0.5 * s, 0.5 * s, 0.95 * s), (0.03, 0.02, -1)), 0.05, FAR),
        ("inside-diag", look((0.9 * s, 0.45 * s, 0.1 * s), (-0.8, 0.1, 0.6)), 0.05, FAR),
        ("cavity", look((0.40 * s, 0.40 * s, 0.58 * s), (0.5, 0.6, -0.6)), 0.02, FAR),
        ("in-solid", look((0.16 * s, 0.20 * s, 0.80 * s), (0.6, 0.3, -0.7)), 0.02, FAR),
        ("roll30", look((0.5 * s, 0.5 * s, -0.3 * s), (0.05, 0.02, 1), roll_deg=30.0), NEAR, FAR),
        ("roll90-z", look((0.45 * s, 0.55 * s, 1.3 * s), (0.0, 0.03, -1), roll_deg=90.0), NEAR, FAR),
        ("far", look((4.5 * s, 3.0 * s, -9.0 * s), (-4.0, -2.5, 9.5)), NEAR, 30.0 * s),
        ("near-far-cut", look((0.5 * s, 0.5 * s, -0.3 * s), (0, 0.01, 1)), 0.62 * s, 0.86 * s),
        ("graze-y", look((-0.2 * s, 0.30 * s, 0.5 * s), (1, 0.0, 0.0)), NEAR, FAR),
        ("axes-z", axes((1, 2, 3), (0.5 * s, 0.5 * s, -0.3 * s)), NEAR, FAR),
        ("axes-neg-z", axes((-1, 2, -3), (0.5 * s, 0.5 * s, 1.3 * s)), NEAR, FAR),
        ("axes-x", axes((3, 2, -1), (0.5 * s, 0.45 * s, 0.5 * s)), 0.05, FAR),          # inside, looking along -x: dir.z = -cam x
        ("axes-y", axes((1, -3, 2), (0.55 * s, 0.1 * s, 0.5 * s)), 0.05, FAR),          # looking along +y: dir.z = -cam y (zero on row cy)
        ("macro-plane", axes((-1, 2, -3), mp), 0.02, FAR),                          # origin on macro-cell faces (exact at 128^3 @ 4 m)
        ("away", look((0.5 * s, 0.5 * s, -0.3 * s), (0, 0, -1)), NEAR, FAR),            # nothing in sight
        ("out-of-solid", look((0.95 * s, 0.75 * s, 0.70 * s), (1, 0.05, 0.02)), 0.02, FAR),   # inside the +x box, towards the volume's face
    ]
    return v


ZERO_HIT_VIEWS = ("away", "out-of-solid")


# ---- the fused volume ------------------------------------------------------------------------------------------------------------------------------
FUSED_RES, FUSED_SIZE = 104, 3.0
FUSED_TRUNC = 5 * FUSED_SIZE / FUSED_RES


def fused_frames():
    """[(pose float32, depth mm)]: Scene S from the standard trajectory, from the +x side and from behind (looking along -z)"""
    s = FUSED_SIZE
    poses = [S.trajectory_pose(k, s) for k in (0, 3, 6)]
    poses += [look((1.05 * s, 0.5 * s, 0.5 * s), (-1, 0.02, 0.01)), look((1.02 * s, 0.47 * s, 0.55 * s), (-1, 0.0, -0.04))]
    poses += [look((0.5 * s, 0.52 * s, 1.05 * s), (0.01, 0.0, -1)), look((0.47 * s, 0.5 * s, 1.08 * s), (0.03, -0.02, -1))]
    out = []
    for p in poses:
        p32 = p.astype(np.float32)
        out.append((p32, S.render_depth_mm(p32, RAGGED, s)))
    return out


def fuse_oracle():
    ovol = O.OVolume(FUSED_RES, FUSED_SIZE, P["volume_max_weight"])
    ocam = O.Cam.make(*RAGGED)
    for pose, mm in fused_frames():
        tr = O.trunc_depth(O.depth_mm_to_m(mm), NEAR, FAR)
        n = O.vertices_to_normals(O.depth_to_vertices(O.bilateral(tr, P["filter_sigma_pixel"], P["filter_sigma_depth"]), ocam))
        O.integrate(ovol, tr, n, None, False, False, pose, FUSED_TRUNC, 4.0, ocam, ocam)
    return ovol


def fuse_gpu(ctx):
    for pose, mm in fused_frames():
        ctx.upload_depth_mm(mm)
        ctx.preprocess(NEAR, FAR, P["filter_sigma_pixel"], P["filter_sigma_depth"])
        ctx.integrate(pose, FUSED_TRUNC, 4.0)


# ---- the scenarios ---------------------------------------------------------------------------------------------------------------------------------
# (volume id, res, size, colour, [(camera, view names or None = all)])
_FEW = ("front+z", "back-z", "corner-mixed", "inside-diag", "far", "axes-neg-z")
VOLUMES = [
    ("a104", 104, 3.0, False, [(RAGGED, None), (ODD, ("axes-z", "axes-neg-z", "axes-x", "axes-y", "macro-plane", "graze-y"))]),
    ("a128", 128, 4.0, False, [(RAGGED, None), (ODD, ("axes-z", "axes-neg-z", "axes-x", "axes-y", "macro-plane", "graze-y"))]),
    ("a384", 384, 3.0, False, [(RAGGED, None), (VGA, _FEW)]),
    ("c64", 64, 3.0, True, [(RAGGED, ("front+z", "back-z", "side-x", "corner-mixed", "inside-diag", "roll30", "axes-y"))]),
    ("fused", FUSED_RES, FUSED_SIZE, False, [(RAGGED, None)]),
]


def inc_for(res, size):
    return P["raycast_increment_factor"] * 5 * size / res


def calls(vol):
    """[(key, camera, view name, pose float32, near, far)] of one volume, in the order both sides cast them"""
    vid, res, size, _, cams = vol
    vs = views(size, res)
    out = []
    for cam in cams:
        for name, pose, near, far in vs:
            if cam[1] is None or name in cam[1]:
                out.append(("%s/%dx%d/%s" % (vid, cam[0][0], cam[0][1], name), cam[0], name, pose.astype(np.float32), near, far))
    return out


def volume_data(vol):
    vid, res, size, color, _ = vol
    if vid == "fused":
        ov = fuse_oracle()
        return ov.tsdf.copy(), ov.weight.copy(), None
    return analytic_volume(res, size, color)


def oracle_volume(vol, data):
    vid, res, size, color, _ = vol
    ov = O.OVolume(res, size, P["volume_max_weight"])
    ov.tsdf[:] = data[0]
    ov.weight[:] = data[1]
    if data[2] is not None:
        ov.color[:] = data[2]
    return ov


def oracle_maps(vol, ovol, call):
    """the oracle's maps of one call: vertices, normals, rgb and levels 1-2 of the two pyramids"""
    _, cam, _, pose, near, far = call
    res, size, color = vol[1], vol[2], vol[3]
    ov, on, orgb = O.raycast(ovol, color, pose, inc_for(res, size), O.Cam.make(*cam), near, far)
    pv, pn = O.pyramid(ov, 3), O.pyramid(on, 3, normals=True)
    return dict(v=ov, n=on, rgb=orgb if color else None, v1=pv[1], v2=pv[2], n1=pn[1], n2=pn[2])


def hits(n):
    return int((np.abs(n[..., :3]).sum(axis=-1) > 0).sum())


# minimum hits per view (any volume, any camera: a fraction of the smallest count the oracle gives at the smallest camera); the zero-hit views: exactly 0
def min_hits(view, cam):
    if view in ZERO_HIT_VIEWS:
        return 0
    if view in ("far",):
        return 20
    return 150 if cam == ODD else 400 if cam == RAGGED else 4000
