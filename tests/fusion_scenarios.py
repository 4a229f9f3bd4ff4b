"""The frames of tests/test_gpu_fusion_forms.py: what its child process (fusion_forms_child.py) fuses on the GPU and what the parent fuses with the
CPU oracle.  Both sides build every frame's input here, so the two can only differ in the fusion itself."""
import numpy as np

import oracle_lib as O
from hybkinectfu_amd import scene as S

P = S.STOCK
RAGGED = (203, 151, 101.0, 75.0, 166.5, 166.5)          # no multiple of any tile or wave the kernels use
MID = (160, 120, 79.5, 59.5, 131.25, 131.25)
VGA_RGB = (640, 480, 319.5, 239.5, 525.0, 525.0)         # the reference projects into the colour image with 525 / 320 / 240 (integrateVolume.cu:56-57)


def _f(k, defer=None, trunc=0.1, dist=4.0, holes=0, color=False, angled=False, layers=False):
    return dict(k=k, defer=defer, trunc=trunc, dist=dist, holes=holes, color=color, angled=angled, layers=layers)


# Res 104 = 13 bricks per axis: the last macro cell of every row is partial.  max_weight 3 saturates free space after three frames; deferral on in the
# middle, off at the end (the pending counts are flushed in front of the plain kernel); far views cut into the deferred space at the frustum's edges,
# sensor drop-outs leave partial waves, a wide band turns free space into band voxels, a short integration distance rebuilds the tile tables.
_S1 = [_f(0, 0), _f(1, 1), _f(2, 1), _f(3, 1), _f(4, 1, layers=True), _f(40, 1), _f(76, 1, holes=40), _f(21, 1, trunc=0.25), _f(22, 1, dist=1.2),
       _f(5, 0), _f(6, 0, layers=True), _f(77, 0, holes=40), _f(7, 0)]
_T4 = 5 * 3.0 / 64

SCENARIOS = {
    "S1": dict(res=104, size=3.0, maxw=3.0, cam=RAGGED, frames=_S1),
    "S2": dict(res=40, size=3.0, maxw=128.0, cam=MID, frames=[_f(0, 1), _f(1, 1), _f(41, 1, holes=30), _f(2, 0)]),
    # a z-slab of S1's volume: stored layers 16 .. 88 (brick layers 2 .. 11, bz0 != 0, partial macro cells at both ends), owned 24 .. 80
    "S3": dict(res=104, size=3.0, maxw=3.0, cam=RAGGED, slab=(24, 80), halo=8, frames=_S1),
    # colour through the VGA colour camera, angle weight off and on, between deferred frames without colour
    "S4": dict(res=64, size=3.0, maxw=P["volume_max_weight"], cam=MID, rcam=VGA_RGB, has_color=True,
               frames=[_f(0, 1, _T4, 2.5, color=True), _f(1, 1, _T4, 2.5), _f(2, 1, _T4, 2.5), _f(3, 1, _T4, 2.5, color=True, angled=True),
                       _f(4, 1, _T4, 2.5), _f(5, 1, _T4, 2.5, color=True), _f(6, 1, _T4, 2.5, color=True, angled=True)]),
    # the device-resident pose: kf_icp_track, then kf_integrate_volume(transform = NULL), whose cull the tracking launch has run as its tail
    "S5": dict(res=104, size=3.0, maxw=P["volume_max_weight"], cam=RAGGED, tracked=True,
               frames=[_f(0, 0, 5 * 3.0 / 104, 2.5), _f(3, 0, 5 * 3.0 / 104, 2.5), _f(6, 0, 5 * 3.0 / 104, 2.5)]),
}
ORDER = ("S1", "S2", "S3", "S4", "S5")


def stored_range(sc):
    """the layers a context of this scenario stores (kf_stored_z_range): the slab widened by the halo to whole bricks, clipped"""
    if "slab" not in sc:
        return 0, sc["res"]
    z0, z1 = sc["slab"]
    hb = -(-sc["halo"] // 8)
    return max(0, (z0 // 8 - hb) * 8), min(sc["res"], (z1 // 8 + hb) * 8)


def owned_range(sc):
    return sc.get("slab", (0, sc["res"]))


def frame_inputs(name, sc, i):
    """frame i of a scenario: (pose, depth in mm, rgb or None, gated depth in m, normals) -- the normals are the oracle's on both sides (the
    colour kernels read them for the angle weight; the bilateral filters differ in last bits)"""
    fr, cam = sc["frames"][i], sc["cam"]
    pose = S.trajectory_pose(fr["k"], sc["size"]).astype(np.float32)
    mm = S.render_depth_mm(pose, cam, sc["size"])
    if fr["holes"]:
        mm = mm.copy()
        mm.reshape(-1)[np.random.default_rng(fr["k"]).integers(0, mm.size, fr["holes"])] = 0
    rgb = None
    if fr["color"]:
        rc = sc["rcam"]
        rgb = np.random.default_rng(1000 * ORDER.index(name) + i).integers(0, 256, (rc[1], rc[0], 3)).astype(np.uint8)
    ocam = O.Cam.make(*cam)
    tr = O.trunc_depth(O.depth_mm_to_m(mm), P["depth_trunc_min"], P["depth_trunc_max"])
    n = O.vertices_to_normals(O.depth_to_vertices(O.bilateral(tr, P["filter_sigma_pixel"], P["filter_sigma_depth"]), ocam))
    return pose, mm, rgb, tr, n


def oracle_run(name, sc, poses=None):
    """the scenario through the CPU oracle: per-frame update counts and observed-voxel counts (owned layers), the final planes of the stored layers.
    poses: the device-resident poses the GPU tracked (S5), in place of the trajectory's"""
    z0, z1 = stored_range(sc)
    o0, o1 = owned_range(sc)
    ovol = O.OVolume(sc["res"], sc["size"], sc["maxw"])
    ocam = O.Cam.make(*sc["cam"])
    orcam = O.Cam.make(*sc["rcam"]) if "rcam" in sc else ocam
    upd, gt0 = [], []
    for i, fr in enumerate(sc["frames"]):
        pose, mm, rgb, tr, n = frame_inputs(name, sc, i)
        if poses is not None:
            pose = poses[i]
        upd.append(O.integrate(ovol, tr, n, rgb, fr["color"], fr["angled"], pose, fr["trunc"], fr["dist"], ocam, orcam, z0, z1))
        gt0.append(int((ovol.weight[o0:o1] > 0).sum()))
    return dict(upd=np.array(upd, np.uint64), gt0=np.array(gt0, np.int64), tsdf=ovol.tsdf[z0:z1].copy(), weight=ovol.weight[z0:z1].copy(),
                color=ovol.color[z0:z1].copy() if sc.get("has_color") else None)
