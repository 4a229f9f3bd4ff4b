"""GPU: colour on z-slabs.  Slab contexts through the colour forms of the ray-form merge, colour slab groups (LOCAL, RCCL in child processes, the
full-size C4 geometry) and the C++ class HybKinectfuSlabs with useRGBData reproduce the whole-volume colour context BIT FOR BIT: colour bytes of
the volume, KF_MAP_RAYCAST_RGB, model maps, poses, coloured triangles, the saved mesh.  No tolerances anywhere.

RGB frames are fresh random images from a seeded generator; the scene is scene.render_depth_mm along scene.trajectory_pose.  The depth gate and the
integration gate are 4 m (GATE): with the stock 2 m integration gate the far wall of the 3 m scene is not fused and most of the surface -- and of the
colour -- would lie in one slab; 4 m reaches through the whole volume from the camera 0.3 m in front of it.

What keeps the comparisons from passing vacuously is asserted from the WHOLE-volume context's results (non_vacuous): more than 10 000 coloured
pixels, at least two members owning >= 1 000 coloured pixels each (the owner of a pixel is the member whose layers hold its vertex's voxel layer),
and at least one pixel of the kind the fourth word exists for -- a colour without a normal, or a vertex owned by another member than its crossing."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O
from hybkinectfu_amd import group as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import pipeline as PL
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = S.STOCK
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = P["raycast_increment_factor"] * P["integrate_sdf_trunc"]
GATE = 4.0
NEAR = P["depth_trunc_min"]


@pytest.fixture(autouse=True)
def _close_leaked():
    yield
    for g in G.live_groups():
        g.close()
    for c in K.live_contexts():
        c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rgb_frame(rng, cam):
    return rng.integers(0, 256, (cam[1], cam[0], 3)).astype(np.uint8)


def vertex_layers(wv, res, size):
    """the voxel layer of every vertex of a whole-volume vertex map, as the kernels compute it: (int)(z * res / size) in fp32, clamped"""
    z = wv[..., 2].astype(np.float32)
    return np.clip((z * np.float32(res) / np.float32(size)).astype(np.int32), 0, res - 1)


def non_vacuous(whole, cuts, res, size, need_owners=2):
    """the conditions, from the whole-volume context alone.  Returns (coloured pixels, colour-without-normal pixels, per-member counts)."""
    rgb = whole.download_map(K.MAP_RAYCAST_RGB)
    wv, wn = whole.download_map(K.MAP_MODEL_VERTICES), whole.download_map(K.MAP_MODEL_NORMALS)
    col = rgb.any(axis=-1)
    has_n = (bits(wn)[..., :3] != 0).any(axis=-1)
    assert int(col.sum()) > 10000, int(col.sum())
    # a coloured pixel WITH a normal has its vertex in the map: its owner is the member whose layers hold the vertex's voxel layer
    gz = vertex_layers(wv, res, size)
    owners = [int((col & has_n & (gz >= cuts[i]) & (gz < cuts[i + 1])).sum()) for i in range(len(cuts) - 1)]
    assert sum(1 for c in owners if c >= 1000) >= need_owners, owners
    return int(col.sum()), int((col & ~has_n).sum()), owners


def foreign_from_whole(whole, pose, cuts, res, size, gate=GATE):
    """coloured pixels whose vertex lies in another member's layers than their crossing, from the WHOLE context alone: its RGB, vertex and normal maps
    and its own crossing words (kf_raycast_volume_slab_cross on the whole volume: crossing parameter t and vertex parameter alpha of every ray).  The
    vertex V = org + dir * alpha is in the map where there is a normal, so the crossing sample is org + (V - org) * t / alpha; pixels with a colour and
    no normal are the other kind and are counted there.  The layer of the crossing is rounded here, not by the kernel: a count to print, not to equal."""
    ta = torch.empty((whole.cam.rows, whole.cam.cols), dtype=torch.int64, device="cuda")
    whole.raycast_slab_cross(pose, INC, NEAR, gate, ta.data_ptr())
    whole.sync()
    w = ta.cpu().numpy().view(np.uint64)
    t, alpha = (w >> np.uint64(32)).astype(np.uint32).view(np.float32), (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    col = whole.download_map(K.MAP_RAYCAST_RGB).any(axis=-1)
    wv, wn = whole.download_map(K.MAP_MODEL_VERTICES), whole.download_map(K.MAP_MODEL_NORMALS)
    sel = col & (bits(wn)[..., :3] != 0).any(axis=-1) & np.isfinite(t) & (alpha != 0)
    org_z = np.float32(pose[2, 3] if pose is not None else whole.track_result()[1][2, 3])
    vz = wv[..., 2][sel].astype(np.float32)
    pz = org_z + (vz - org_z) * (t[sel] / alpha[sel])
    layer = lambda z: np.clip((z * np.float32(res) / np.float32(size)).astype(np.int32), 0, res - 1)
    owner = lambda z: np.searchsorted(np.asarray(cuts), layer(z), side="right") - 1
    return int((owner(vz) != owner(pz)).sum())


def whole_color_frame(ctx, mm, rgb, k, gate=GATE):
    if isinstance(mm, np.ndarray):
        ctx.upload_depth_mm(mm)
        ctx.upload_rgb(rgb)
    else:
        ctx.set_depth_mm_device(mm)
        ctx.set_rgb_device(rgb)
    ctx.preprocess(NEAR, gate, P["filter_sigma_pixel"], P["filter_sigma_depth"])
    ctx.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
    ctx.integrate(None, P["integrate_sdf_trunc"], gate, has_color=True, angle_weight=True)
    ctx.raycast(None, INC, NEAR, gate, has_color=True)


def check_color_frame(g, whole, k, tracked=True):
    ok_g, pose_g, st_g, _ = g.track_result(check_lockstep=True)
    ok_w, pose_w, st_w, _ = whole.track_result()
    assert ok_g == ok_w == tracked and st_g == st_w, (k, ok_g, ok_w, st_g, st_w)
    assert np.array_equal(bits(pose_g), bits(pose_w)), k
    wrgb = whole.download_map(K.MAP_RAYCAST_RGB)
    for i, m in enumerate(g.members()):
        ok_m, pose_m, st_m, _ = m.track_result()
        assert ok_m == ok_g and st_m == st_g and np.array_equal(bits(pose_m), bits(pose_w)), (k, i)
        for level in range(3):
            for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                assert np.array_equal(bits(m.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (k, i, level, map_id)
        assert np.array_equal(m.download_map(K.MAP_RAYCAST_RGB), wrgb), (k, i)


def check_color_volume(g, whole):
    tw, ww, cw = whole.download_volume(color=True)
    for m in g.members():
        z0, z1 = m.owned
        t, w, c = m.download_volume(z0, z1, color=True)
        assert np.array_equal(bits(t), bits(tw[z0:z1])) and np.array_equal(w, ww[z0:z1]) and np.array_equal(c, cw[z0:z1]), (z0, z1)
    assert sum(m.stats()["weight_gt0"] for m in g.members()) == whole.stats()["weight_gt0"] == int((ww > 0).sum())
    assert int(np.count_nonzero(cw[ww > 0])) > 10000


def merge_by_hand(slabs, pose, cam, near, far, inc, dev):
    """the colour merge with MIN and SUM in torch: words, 4-word candidates in both uses (equal bits), maps.  Returns (ta per slab, ta_min, cand per slab)."""
    tas, owns, specs = [], [], []
    for c in slabs:
        ta = torch.empty((cam[1], cam[0]), dtype=torch.int64, device=dev)
        own = torch.empty_like(ta)
        spec = torch.full((cam[1], cam[0], 4), 7.0, dtype=torch.float32, device=dev)
        c.raycast_slab_cross_spec_color(pose, inc, near, far, ta.data_ptr(), own.data_ptr(), spec.data_ptr())
        c.sync()
        assert torch.equal(ta, own)
        tas.append(ta); owns.append(own); specs.append(spec)
    ta_min = torch.stack(tas).min(dim=0).values.contiguous()
    acc = torch.zeros((cam[1], cam[0], 4), dtype=torch.int32, device=dev)
    cands = []
    for r, c in enumerate(slabs):
        cand = torch.full((cam[1], cam[0], 4), 7.0, dtype=torch.float32, device=dev)
        cand2 = torch.full((cam[1], cam[0], 4), 9.0, dtype=torch.float32, device=dev)
        c.slab_ray_normals_color(pose, inc, near, far, ta_min.data_ptr(), owns[r].data_ptr(), specs[r].data_ptr(), cand.data_ptr())
        c.slab_ray_normals_color(pose, inc, near, far, ta_min.data_ptr(), None, None, cand2.data_ptr())
        c.sync()
        assert torch.equal(cand.view(torch.int32), cand2.view(torch.int32)), r          # the speculative and the NULL-dev_spec use: the same bits
        acc += cand.view(torch.int32)
        cands.append(cand.view(torch.int32))
    # one contributor per pixel and word
    assert int((torch.stack([(cd != 0).any(dim=-1) for cd in cands]).sum(dim=0) > 1).sum()) == 0
    rays = acc.view(torch.float32).contiguous()
    for c in slabs:
        c.set_model_maps_rays_color(pose, ta_min.data_ptr(), rays.data_ptr())
        c.sync()
    return tas, ta_min, cands


def kinds(tas, ta_min, cands):
    """pixels of the two kinds the fourth word exists for, from the by-hand merge's own buffers: (colour without a normal, contributor that did not meet the crossing)"""
    no_normal = foreign = 0
    for ta, cd in zip(tas, cands):
        contributes = (cd != 0).any(dim=-1)
        no_normal += int(((cd[..., 3] != 0) & ~(cd[..., :3] != 0).any(dim=-1)).sum())
        foreign += int((contributes & (ta != ta_min)).sum())
    return no_normal, foreign


@pytest.mark.parametrize("cuts", [[0, 64, 192], [0, 64, 128, 192]], ids=["two", "three"])
def test_slab_contexts_through_the_c_abi_equal_whole_colour_context(cuts):
    """1. per call, explicit poses: volume incl. colour bytes, the merged maps and the RGB map on every context, both uses of kf_slab_ray_normals_color"""
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    halo = PL.slab_halo_layers(res, size, INC)
    dev = torch.device("cuda", 0)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, has_color=True, max_triangles=900000)
    slabs = [K.Context(kcam, res, size, P["volume_max_weight"], levels=3, has_color=True, slab=(cuts[i], cuts[i + 1]), halo=halo, max_triangles=900000)
             for i in range(len(cuts) - 1)]
    rng = np.random.default_rng(2024)
    total_no_normal = total_foreign = whole_no_normal = 0
    for k in range(4):
        pose = S.trajectory_pose(k, size).astype(np.float32)
        mm, rgb = S.render_depth_mm(pose, cam, size), rgb_frame(rng, cam)
        for c in [whole] + slabs:
            c.upload_depth_mm(mm)
            c.upload_rgb(rgb)
            c.preprocess(NEAR, GATE, P["filter_sigma_pixel"], P["filter_sigma_depth"])
            c.integrate(pose, P["integrate_sdf_trunc"], GATE, has_color=True, angle_weight=True)
        assert all(c.fusion_form()["color"] == 1 for c in [whole] + slabs)
        whole.raycast(pose, INC, NEAR, GATE, has_color=True)
        n_col, n_nn, owners = non_vacuous(whole, cuts, res, size)
        whole_no_normal += n_nn
        n_fo = foreign_from_whole(whole, pose, cuts, res, size)
        tas, ta_min, cands = merge_by_hand(slabs, pose, cam, NEAR, GATE, INC, dev)
        nn, fo = kinds(tas, ta_min, cands)
        total_no_normal += nn; total_foreign += fo
        print("frame %d: coloured %d, per member %s; from the whole context: colour without normal %d, vertex owner != crossing owner %d; "
              "from the slabs' buffers: %d, %d" % (k, n_col, owners, n_nn, n_fo, nn, fo))
        wrgb = whole.download_map(K.MAP_RAYCAST_RGB)
        for i, c in enumerate(slabs):
            for level in range(3):
                for map_id in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS):
                    assert np.array_equal(bits(c.download_map(map_id, level)), bits(whole.download_map(map_id, level))), (k, i, level, map_id)
            assert np.array_equal(c.download_map(K.MAP_RAYCAST_RGB), wrgb), (k, i)
    assert total_no_normal == whole_no_normal                      # (the whole context's own count of such pixels)
    assert whole_no_normal >= 1, whole_no_normal                   # from the whole context alone (the slabs' own counts above are printed, not relied on)
    tw, ww, cw = whole.download_volume(color=True)
    assert int(np.count_nonzero(cw[ww > 0])) > 10000
    for c in slabs:
        z0, z1 = c.owned
        t, w, col = c.download_volume(z0, z1, color=True)
        assert np.array_equal(bits(t), bits(tw[z0:z1])) and np.array_equal(w, ww[z0:z1]) and np.array_equal(col, cw[z0:z1]), (z0, z1)
    # the extraction: slab-major coloured triangles = the whole volume's sequence
    thr = 300 * size / res
    for c in [whole] + slabs:
        c.marching_cubes(thr, has_color=True)
    wt = whole.triangles()
    parts = [c.triangles() for c in slabs]
    assert len(wt) > 1000 and b"".join(t.tobytes() for t in parts) == wt.tobytes()
    coloured = [int((t["v"]["color"] != 0).any(axis=(1, 2)).sum()) for t in parts]
    assert sum(1 for n in coloured if n > 0) >= 2, coloured
    for c in [whole] + slabs:
        c.close()


def test_colour_merge_equals_the_oracle_at_a_small_size():
    """1. (oracle) a 64^3 colour volume fused by the CPU oracle, uploaded into two slab contexts: the by-hand colour merge gives the
    oracle's raycast(has_color=True) -- vertices, normals, colours -- which pins the slab = whole equality from outside"""
    size, res, cam = 3.0, 64, (160, 120, 79.5, 59.5, 131.25, 131.25)
    rcam = S.vga_camera()
    ocam, kcam, orcam, krcam = O.Cam.make(*cam), K.camera(*cam), O.Cam.make(*rcam), K.camera(*rcam)
    trunc = 5 * size / res
    inc = 0.7 * trunc
    ovol = O.OVolume(res, size, P["volume_max_weight"])
    rng = np.random.default_rng(11)
    for k in range(3):
        pose = S.trajectory_pose(3 * k, size).astype(np.float32)
        mm = S.render_depth_mm(pose, cam, size)
        tr = O.trunc_depth(O.depth_mm_to_m(mm), NEAR, GATE)
        n = O.vertices_to_normals(O.depth_to_vertices(O.bilateral(tr, P["filter_sigma_pixel"], P["filter_sigma_depth"]), ocam))
        assert O.integrate(ovol, tr, n, rng.integers(0, 256, (480, 640, 3)).astype(np.uint8), True, True, pose, trunc, GATE, ocam, orcam) > 10000
    ov, on, orgb = O.raycast(ovol, True, pose, inc, ocam, NEAR, GATE)
    assert int(orgb.any(axis=-1).sum()) > 1000
    halo = PL.slab_halo_layers(res, size, inc)
    cuts = [0, 32, 64]
    slabs = [K.Context(kcam, res, size, P["volume_max_weight"], levels=3, has_color=True, rgb_cam=krcam, slab=(cuts[i], cuts[i + 1]), halo=halo)
             for i in range(2)]
    for c in slabs:
        z0, z1 = c.stored
        c.upload_volume(ovol.tsdf[z0:z1], ovol.weight[z0:z1], ovol.color[z0:z1], z0=z0)
    merge_by_hand(slabs, pose, cam, NEAR, GATE, inc, torch.device("cuda", 0))
    for i, c in enumerate(slabs):
        assert np.array_equal(bits(c.download_map(K.MAP_MODEL_VERTICES)), bits(ov)), i
        assert np.array_equal(bits(c.download_map(K.MAP_MODEL_NORMALS)), bits(on)), i
        assert np.array_equal(c.download_map(K.MAP_RAYCAST_RGB), orgb), i
    for c in slabs:
        c.close()


def test_prefetch_note_is_left_alone_by_the_colour_speculation():
    """kf_prefetch_frame followed by the colour form: the speculation launch carries no riders, the note stays and is void at the next kf_preprocess,
    which preprocesses the frame by its own launches -- every output has the bits of a context that never prefetched"""
    size, res, cam = 3.0, 64, (160, 120, 79.5, 59.5, 131.25, 131.25)
    kcam = K.camera(*cam)
    trunc = 5 * size / res
    inc = 0.7 * trunc
    halo = PL.slab_halo_layers(res, size, inc)
    dev = torch.device("cuda", 0)
    a, b = [K.Context(kcam, res, size, P["volume_max_weight"], levels=3, has_color=True, rgb_cam=kcam, slab=(0, res), halo=halo) for _ in range(2)]   # one member owning every layer, as at world 1
    rng = np.random.default_rng(23)
    poses = [S.trajectory_pose(3 * k, size).astype(np.float32) for k in range(3)]
    mms = [torch.from_numpy(S.render_depth_mm(p, cam, size).astype(np.int16)).to(dev) for p in poses]
    rgbs = [torch.from_numpy(rng.integers(0, 256, (cam[1], cam[0], 3)).astype(np.uint8)).to(dev) for _ in poses]
    coloured = 0
    for k, pose in enumerate(poses):
        out = []
        for c in (a, b):
            c.set_depth_mm_device(mms[k].data_ptr())
            c.set_rgb_device(rgbs[k].data_ptr())
            c.preprocess(NEAR, GATE, P["filter_sigma_pixel"], P["filter_sigma_depth"])
            c.integrate(pose, trunc, GATE, has_color=True, angle_weight=True)
            if c is a and k + 1 < len(poses):
                c.prefetch_frame(mms[k + 1].data_ptr(), NEAR, GATE, P["filter_sigma_pixel"], P["filter_sigma_depth"])
            ta = torch.empty((cam[1], cam[0]), dtype=torch.int64, device=dev)
            own = torch.empty_like(ta)
            spec = torch.full((cam[1], cam[0], 4), 7.0, dtype=torch.float32, device=dev)
            c.raycast_slab_cross_spec_color(pose, inc, NEAR, GATE, ta.data_ptr(), own.data_ptr(), spec.data_ptr())
            c.sync()
            assert c.raycast_form()["kernel"] == 1                  # KF_RC_PLAIN: no rider in the colour launch
            out.append((ta, own, spec.view(torch.int32)))
        assert all(torch.equal(x, y) for x, y in zip(*out)), k
        coloured += int((out[1][2][..., 3] != 0).sum())
        for map_id in (K.MAP_FILTERED_DEPTH, K.MAP_NEW_VERTICES, K.MAP_NEW_NORMALS):
            assert np.array_equal(bits(a.download_map(map_id)), bits(b.download_map(map_id))), (k, map_id)
    assert coloured > 1000, coloured
    for x, y in zip(a.download_volume(color=True), b.download_volume(color=True)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    a.close()
    b.close()


def _probe_cuts(res, size, world):
    cam = S.vga_camera()
    first = torch.from_numpy(S.render_depth_mm(S.trajectory_pose(0, size), cam, size).astype(np.int16)).cuda()
    work = PL.probe_layer_work(K.camera(*cam), res, size, None, first.data_ptr(), probe_res=64)
    ranges = PL.slab_ranges(res, world, work, halo=PL.slab_halo_layers(res, size, INC))
    return [0] + [r[1] for r in ranges]


@pytest.mark.parametrize("cuts", [[0, 64, 128, 192], "probe4"], ids=["even3", "probe4"])
def test_local_colour_group_equals_whole_volume(cuts):
    """2. six tracked frames: every frame and member pose bits, verdict, model maps (levels 0-2), RGB map; at the end the volume incl. colour, the
    observed-voxel counts and the coloured triangle sequence"""
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    if cuts == "probe4":
        cuts = _probe_cuts(res, size, 4)
    params = G.stock_params(trunc_max=GATE, integ_dist=GATE)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, max_triangles=900000, has_color=True)
    whole.set_pose(S.pose0(size))
    g = G.Group.local(kcam, res, size, cuts, max_triangles=900000, params=params, has_color=True, angle_weight=True)
    assert g.halo == PL.slab_halo_layers(res, size, INC) and len(g.members()) == len(cuts) - 1
    rng = np.random.default_rng(7)
    no_normal = 0
    for k in range(6):
        mm, rgb = S.render_depth_mm(S.trajectory_pose(k, size), cam, size), rgb_frame(rng, cam)
        whole_color_frame(whole, mm, rgb, k)
        g.frame(mm, k, rgb=rgb)                                     # host frames: one copy each into the group's buffers
        check_color_frame(g, whole, k)
        n_col, n_nn, owners = non_vacuous(whole, cuts, res, size)
        no_normal += n_nn
        print("frame %d: coloured %d, per member %s, colour without normal %d, vertex owner != crossing owner %d"
              % (k, n_col, owners, n_nn, foreign_from_whole(whole, None, cuts, res, size)))
    assert no_normal >= 1                                          # pixels whose colour travels without a normal
    check_color_volume(g, whole)
    thr = 300 * size / res
    whole.marching_cubes(thr, has_color=True)
    g.marching_cubes(thr)
    wt, gt = whole.triangles(), g.triangles()
    assert len(wt) > 1000 and gt.tobytes() == wt.tobytes()
    coloured = [int((m.triangles()["v"]["color"] != 0).any(axis=(1, 2)).sum()) for m in g.members()]
    print("coloured triangles per member", coloured)
    assert sum(1 for c in coloured if c > 0) >= 2, coloured
    ends = np.cumsum([m.triangles().shape[0] for m in g.members()])
    win = np.zeros(10, dtype=K.TRI_DTYPE)
    inner = [int(e) for e in ends[:-1] if 5 <= e <= len(wt) - 5]
    assert inner
    for e in inner:                                                 # windows across member boundaries
        assert G.load().kf_group_read_triangles(g.h, win.ctypes.data_as(C.c_void_p), e - 5, 10) == 0
        assert win.tobytes() == wt[e - 5:e + 5].tobytes()
    g.close()
    whole.close()


def test_lost_frame_keeps_colour_members_in_lock_step():
    """3. an all-zero depth frame is lost by every member alike: nothing is fused, and colour planes and RGB maps stay equal to the whole context's"""
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    params = G.stock_params(trunc_max=GATE, integ_dist=GATE)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, has_color=True)
    whole.set_pose(S.pose0(size))
    g = G.Group.local(kcam, res, size, [0, 72, 192], params=params, has_color=True)
    zero = np.zeros((cam[1], cam[0]), np.uint16)
    seq = [S.render_depth_mm(S.trajectory_pose(k, size), cam, size) for k in range(3)] + [zero] + \
          [S.render_depth_mm(S.trajectory_pose(k, size), cam, size) for k in range(3, 5)]
    rng = np.random.default_rng(3)
    for k, mm in enumerate(seq):
        rgb = rgb_frame(rng, cam)
        if k == 3:
            before = [(m.stats(), m.download_volume(color=True)) for m in g.members()]
        whole_color_frame(whole, mm, rgb, k)
        g.frame(mm, k, rgb=rgb)
        check_color_frame(g, whole, k, tracked=(k != 3))
        if k == 3:
            for m, (st0, (t0, w0, c0)) in zip(g.members(), before):
                st = m.stats()
                assert st["frames_lost"] == st0["frames_lost"] + 1 and st["frames_fused"] == st0["frames_fused"], (st0, st)
                t, w, c = m.download_volume(color=True)
                assert np.array_equal(bits(t), bits(t0)) and np.array_equal(w, w0) and np.array_equal(c, c0)
            assert whole.stats()["frames_lost"] == 1
        else:
            non_vacuous(whole, [0, 72, 192], res, size, need_owners=1)
    check_color_volume(g, whole)
    g.close()
    whole.close()


def _child(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k == "KF_STATS_CROSSCHECK"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_color_rccl_child.py"), mode], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "group colour rccl ok" in r.stdout, "child %s exited with %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_rccl_all_world1_with_colour_equals_plain_colour_context():
    _child("all1")


def test_rccl_rank_world1_with_colour_equals_plain_colour_context():
    _child("rank1")


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason="needs two or more visible devices")
def test_rccl_all_with_colour_over_every_visible_device():
    _child("alldev")


def test_cpp_slab_class_with_rgb_equals_hybkinectfu_with_rgb(tmp_path):
    """5. HybKinectfuSlabs with useRGBData (LOCAL, 2 members) against HybKinectfu with useRGBData, five frames: pose bits, the saveMesh .ply files byte
    for byte, vertex colours in the file; a frame without a BGR image is refused"""
    cam = S.vga_camera()
    res, size = 192, 3.0
    app = H.App(res, size, cam, max_triangles=900000, use_rgb=True, integrate_dist=GATE, trunc_max=GATE)
    sl = C.CDLL(os.path.join(K.PKG_DIR, "libhybkf_slabs.so"))
    cuts = (C.c_uint32 * 3)(0, 96, 192)
    sl.hkf_slabs_configure_color(1, 1)
    try:
        assert sl.hkf_slabs_init(res, C.c_float(size), cam[0], cam[1], C.c_float(cam[2]), C.c_float(cam[3]), C.c_float(cam[4]), C.c_float(cam[5]),
                                 900000, C.c_float(0), C.c_float(GATE), C.c_float(GATE), 0, G.LOCAL, 2, cuts, None, 0) == 0
        rng = np.random.default_rng(5)
        for k in range(5):
            mm = np.ascontiguousarray(S.render_depth_mm(S.trajectory_pose(k, size), cam, size), np.uint16)
            rgb = rgb_frame(rng, cam)
            assert app.h.hkf_app_process_frame_color(mm.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), k, C.c_double(0.0)) == 1
            assert sl.hkf_slabs_process_frame_color(mm.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), 0, k) == 1
            ok_a, pa = app.pose()
            ps = np.zeros(16, np.float32)
            assert ok_a and sl.hkf_slabs_get_pose(ps.ctypes.data_as(C.c_void_p)) == 1
            assert np.array_equal(bits(ps.reshape(4, 4)), bits(pa)), k
        assert sl.hkf_slabs_process_frame(mm.ctypes.data_as(C.c_void_p), 0, 5) == -2           # useRGBData and no BGR image: refused, nothing fused
        n = app.generate_mesh()
        assert n > 1000 and sl.hkf_slabs_generate_mesh() == n
        fa, fs = str(tmp_path / "whole.ply"), str(tmp_path / "slabs.ply")
        nv, nf = C.c_uint32(), C.c_uint32()
        ok, nva, nfa = app.save_mesh(fa)
        assert ok and sl.hkf_slabs_save_mesh(fs.encode(), C.byref(nv), C.byref(nf)) == 1
        assert (nv.value, nf.value) == (nva, nfa) and nfa > 1000
        da, ds = open(fa, "rb").read(), open(fs, "rb").read()
        assert da == ds
        head = ds[:ds.index(b"end_header")].decode("ascii", "replace")
        assert "red" in head and "green" in head and "blue" in head, head
        mesh = H.app_mesh()
        assert len(mesh["colors"]) == nva and int((mesh["colors"][:, :3] != 0).any(axis=1).sum()) > 1000
    finally:
        sl.hkf_slabs_shutdown()
        sl.hkf_slabs_configure_color(0, 1)
        app.close()


def test_c4_eight_colour_members_full_size_on_one_gpu():
    """6. the C4 geometry with colour: 1024^3 @ 6 m, eight LOCAL members, halo 8, two frames beside the whole colour volume (~26 GB), in a child process
    under its own time limit (group_color_c4_child.py runs c4_eight_colour_members below)"""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_color_c4_child.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "group colour c4 ok" in r.stdout, "child exited with %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def c4_eight_colour_members():
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size, gate = 1024, 6.0, 6.0
    cuts = list(range(0, res + 1, 128))
    params = G.stock_params(trunc_max=gate, integ_dist=gate)
    whole = K.Context(kcam, res, size, P["volume_max_weight"], levels=3, has_color=True)
    whole.set_pose(S.pose0(size))
    g = G.Group.local(kcam, res, size, cuts, halo=8, params=params, has_color=True)
    rng = np.random.default_rng(1)
    for k in range(2):
        mm = torch.from_numpy(S.render_depth_mm(S.trajectory_pose(k, size), cam, size).astype(np.int16)).cuda()
        rgb = torch.from_numpy(rgb_frame(rng, cam)).cuda()
        whole_color_frame(whole, mm.data_ptr(), rgb.data_ptr(), k, gate)
        g.frame(mm.data_ptr(), k, rgb=rgb.data_ptr())
        check_color_frame(g, whole, k)
        n_col, n_nn, owners = non_vacuous(whole, cuts, res, size)
        print("frame %d: coloured %d, per member %s, colour without normal %d" % (k, n_col, owners, n_nn))
        g.sync()
        torch.cuda.synchronize()
    assert all(m.fusion_form()["color"] == 1 and m.fusion_form()["defer"] == 0 for m in g.members())    # colour: the plain fusion kernel
    observed = 0
    for z0, z1 in ((120, 136), (504, 520), (888, 904)):             # the planes around three member boundaries, colour included
        tw, ww, cw = whole.download_volume(z0, z1, color=True)
        observed += int((ww > 0).sum())
        for m in g.members():
            a, b = max(z0, m.owned[0]), min(z1, m.owned[1])
            if a < b:
                t, w, c = m.download_volume(a, b, color=True)
                assert np.array_equal(bits(t), bits(tw[a - z0:b - z0])) and np.array_equal(w, ww[a - z0:b - z0]) and \
                    np.array_equal(c, cw[a - z0:b - z0]), (m.owned, a, b)
    assert observed > 0
    g.close()
    whole.close()


def test_wrong_kind_frame_calls_are_refused_without_a_collective():
    """7. a colour group's frame() without RGB and a colourless group's frame(rgb=...) return KF_GROUP_ERR_STATE; nothing was enqueued (no frame fused
    or lost, no merge timed) and the group goes on working"""
    cam = S.vga_camera()
    kcam = K.camera(*cam)
    res, size = 192, 3.0
    mm = S.render_depth_mm(S.trajectory_pose(0, size), cam, size)
    rgb = rgb_frame(np.random.default_rng(0), cam)
    dmm, drgb = torch.from_numpy(mm.astype(np.int16)).cuda(), torch.from_numpy(rgb).cuda()
    for color in (True, False):
        g = G.Group.local(kcam, res, size, [0, 96, 192], has_color=color)
        g.merge_timing(True)
        for call in ((lambda: g.frame(mm, 0)), (lambda: g.frame(dmm.data_ptr(), 0)), (lambda: g.frame_members([dmm.data_ptr()] * 2, 0))) if color else \
                    ((lambda: g.frame(mm, 0, rgb=rgb)), (lambda: g.frame(dmm.data_ptr(), 0, rgb=drgb.data_ptr())),
                     (lambda: g.frame_members([dmm.data_ptr()] * 2, 0, rgb_ptrs=[drgb.data_ptr()] * 2))):
            with pytest.raises(G.GroupError) as e:
                call()
            assert e.value.status == G.ERR_STATE
        g.sync()
        assert g.merge_ms()[1] == 0
        for m in g.members():
            st = m.stats()
            assert st["frames_fused"] == 0 and st["frames_lost"] == 0
        g.frame(mm, 0, rgb=rgb if color else None)                 # the right kind still works: the refusals left the group usable
        ok, _, _, _ = g.track_result(check_lockstep=True)
        assert ok and g.merge_ms()[1] == 1
        g.close()
