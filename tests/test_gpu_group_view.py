"""GPU: the merged view over slab groups -- kf_group_render_view and its three per-member steps (kf_view_slab_cross, kf_view_slab_normals,
kf_view_from_rays) -- against the CPU oracle's whole-volume raycast pushed through the numpy restatement of the byte formulas (view_expect.py).

The volumes and viewpoints are those of raycast_scenarios.py; members are filled through kf_group_member -> Context.borrow -> upload_volume of each
member's stored range.  Pictures are compared byte for byte and the optional float4 maps bit for bit; there is no tolerance anywhere.  A merged view
is a bystander to the group's frames: pose bits, launch forms, kf_get_raycast_form's records, model maps and volumes are the same with and without it."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O
import raycast_scenarios as R
import view_expect as V
from hybkinectfu_amd import group as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = R.P
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIG = (416, 304, 207.5, 151.5, 340.0, 340.0)           # larger than the groups' cameras both ways
ONE = (1, 1, 0.0, 0.0, 82.0, 82.0)                     # one pixel: its ray is the camera's axis
MODES = (K.VIEW_NORMALS, K.VIEW_SHADED, K.VIEW_COLOR)
LAYOUTS = ([0, 56, 104], [0, 40, 72, 104], [0, 104])


@pytest.fixture(autouse=True)
def _close_leaked_groups():
    """a failed test's group is closed, and the tests' device buffers (many start as NaN) go back to the driver: what runs later in the process
    finds no group, no member context and none of this file's memory in torch's cache"""
    yield
    for g in G.live_groups():
        g.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _volume(vid):
    vol = next(v for v in R.VOLUMES if v[0] == vid)
    data = R.volume_data(vol)
    return vol, data, R.oracle_volume(vol, data)


@functools.lru_cache(maxsize=None)
def _want(vid, key, cam):
    """the oracle's maps of one call of the scenarios, at `cam`; computed once, shared, never written"""
    vol, _, ovol = _volume(vid)
    call = next(c for c in R.calls(vol) if c[0] == key)
    return R.oracle_maps(vol, ovol, (key, cam) + call[2:])


def _ragged_calls(vid):
    return [c for c in R.calls(_volume(vid)[0]) if c[1] == R.RAGGED]


def _group(vid, cam, cuts):
    """a LOCAL group over the analytic volume, at the scenarios' increment"""
    vol, data, _ = _volume(vid)
    _, res, size, color, _ = vol
    params = G.stock_params()
    params.raycast = K.RaycastParams(R.inc_for(res, size))
    g = G.Group.local(K.camera(*cam), res, size, cuts, params=params, has_color=color)
    _fill(g, data, color)
    return g


def _fill(g, data, color=False):
    for m in g.members():
        s0, s1 = m.stored
        m.upload_volume(data[0][s0:s1], data[1][s0:s1], data[2][s0:s1] if color else None)


def _render(g, mode, pose, cam, near, far, maps=True):
    dv = dn = None
    if maps:
        dv = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
        dn = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()                                    # (the fills run on torch's stream, the view on the group's)
    g.render_view(mode, pose, K.camera(*cam), near, far, dv.data_ptr() if maps else None, dn.data_ptr() if maps else None)
    img = g.read_view()
    assert g.view_size() == (cam[0], cam[1]) and img.shape == (cam[1], cam[0], 4) and g.view_device()
    return img, (dv.cpu().numpy() if maps else None), (dn.cpu().numpy() if maps else None)


def _check(key, mode, img, gv, gn, want, pose):
    if gv is not None:
        assert np.array_equal(_bits(gv), _bits(want["v"])), (key, mode)
        assert np.array_equal(_bits(gn), _bits(want["n"])), (key, mode)
    exp = V.view_bytes(mode, want["v"], want["n"], rgb=want["rgb"], eye=pose[:3, 3])
    assert np.array_equal(img, exp), (key, mode, int((img != exp).any(axis=-1).sum()))


@pytest.mark.parametrize("cuts", LAYOUTS, ids=["two", "three", "one"])
def test_merged_view_from_every_side_equals_the_oracle(cuts):
    """a104: the group is created with the ODD camera and the views are rendered with RAGGED -- another size, no multiple of the ray tile"""
    vol, data, _ = _volume("a104")
    calls = _ragged_calls("a104")
    assert len(calls) == len(R.views(vol[2], vol[1]))
    g = _group("a104", R.ODD, cuts)
    plain = None
    if len(cuts) == 2:
        plain = K.Context(K.camera(*R.ODD), vol[1], vol[2], P["volume_max_weight"], levels=3)
        plain.upload_volume(data[0], data[1])
    falling = 0
    for key, cam, view, pose, near, far in calls:
        want = _want("a104", key, cam)
        for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
            img, gv, gn = _render(g, mode, pose, cam, near, far)
            _check(key, mode, img, gv, gn, want, pose)
            n_hit = int((img[..., 3] == 255).sum())
            assert n_hit == int((want["v"][..., 3] == 1.0).sum()) and R.hits(gn) >= R.min_hits(view, cam), (key, n_hit)
            if view in R.ZERO_HIT_VIEWS:
                assert n_hit == 0, key
            if plain is not None:
                plain.render_view(mode, pose, K.camera(*cam), R.inc_for(vol[1], vol[2]), near, far)
                assert np.array_equal(img, plain.read_view()), (key, mode)
        falling += int(pose[2, 2] < 0)
    assert falling >= 3, falling
    if plain is not None:
        plain.close()
    g.close()


def _by_hand(members, kcam, cam, pose, inc, near, far, color=False):
    """the three per-member calls and the two reductions by hand, as test_gpu_raycast_sides._merge does for the model maps; returns what each step left"""
    w = 4 if color else 3
    tas, owns, specs, cands = [], [], [], []
    for c in members:
        ta, own = torch.empty((cam[1], cam[0]), dtype=torch.int64, device=DEV), torch.empty((cam[1], cam[0]), dtype=torch.int64, device=DEV)
        spec = torch.full((cam[1], cam[0], w), float("nan"), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()                                    # (the fills run on torch's stream, the members on the group's)
        c.view_slab_cross(color, pose, kcam, inc, near, far, ta.data_ptr(), own.data_ptr(), spec.data_ptr())
        tas.append(ta); owns.append(own); specs.append(spec)
    for c in members:
        c.sync()
    ta_min = torch.stack(tas).min(dim=0).values.contiguous()
    acc = torch.zeros((cam[1], cam[0], w), dtype=torch.int32, device=DEV)
    for c, own, spec in zip(members, owns, specs):
        cand = torch.full((cam[1], cam[0], w), float("nan"), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        c.view_slab_normals(color, pose, kcam, inc, near, far, ta_min.data_ptr(), own.data_ptr(), spec.data_ptr(), cand.data_ptr())
        c.sync()
        acc += cand.view(torch.int32)
        cands.append(cand)
    return ta_min, owns, specs, acc.view(torch.float32).contiguous()


@pytest.mark.parametrize("cuts", LAYOUTS[:2], ids=["two", "three"])
def test_the_vertex_owner_is_not_always_the_crosser(cuts):
    """both layouts cut through the scene's sphere and shell: a crossing's negative sample and its vertex often lie in different members.  Pixels
    where a member's own word won, its speculation is all-zero and the final normal is not show that the owner's path ran."""
    vol, _, _ = _volume("a104")
    _, res, size, _, _ = vol
    inc = R.inc_for(res, size)
    reach = int(np.ceil(inc / (size / res)))                       # a crossing's negative sample lies at most this many layers past its vertex
    g = _group("a104", R.ODD, cuts)
    kcam = K.camera(*R.RAGGED)
    for name in ("front+z", "back-z"):
        key, cam, view, pose, near, far = next(c for c in _ragged_calls("a104") if c[2] == name)
        want = _want("a104", key, cam)
        # the oracle first: the scene has hits whose vertex lies just on the near side of an inner cut, the crossing's sample beyond it
        hit = want["v"][..., 3] == 1.0
        layer = np.floor(want["v"][..., 2] * np.float32(res) / np.float32(size)).astype(np.int64)
        near_cut = np.zeros_like(hit)
        for cut in cuts[1:-1]:
            near_cut |= (layer >= cut - reach) & (layer < cut) if pose[2, 2] > 0 else (layer >= cut) & (layer < cut + reach)
        assert int((hit & near_cut).sum()) >= 1, (cuts, name)
        ta_min, owns, specs, rays = _by_hand(g.members(), kcam, cam, pose, inc, near, far)
        final = (rays.view(torch.int32) != 0).any(dim=-1)
        split = 0
        for own, spec in zip(owns, specs):
            won = (own == ta_min) & ((ta_min >> 32) != 0x7F800000)
            split += int((won & (spec.view(torch.int32) == 0).all(dim=-1) & final).sum())
        assert split >= 1, (cuts, name, split)
        # ... and the picture of those buffers is the oracle's, with the optional maps
        m0 = g.members()[0]
        dv = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
        dn = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        m0.view_from_rays(K.VIEW_SHADED, pose, kcam, ta_min.data_ptr(), rays.data_ptr(), 3, dv.data_ptr(), dn.data_ptr())
        _check(key, K.VIEW_SHADED, m0.read_view(), dv.cpu().numpy(), dn.cpu().numpy(), want, pose)
        # without the speculation every owned vertex is evaluated by kf_view_slab_normals itself: the same candidates
        acc = torch.zeros((cam[1], cam[0], 3), dtype=torch.int32, device=DEV)
        for c in g.members():
            cand = torch.full((cam[1], cam[0], 3), float("nan"), dtype=torch.float32, device=DEV)
            torch.cuda.synchronize()
            c.view_slab_normals(False, pose, kcam, inc, near, far, ta_min.data_ptr(), None, None, cand.data_ptr())
            c.sync()
            acc += cand.view(torch.int32)
        assert torch.equal(acc, rays.view(torch.int32)), (cuts, name)
    g.close()


def test_view_slab_cross_at_the_contexts_camera_equals_the_frame_calls():
    """whenever view_cam is the context's camera: the words, their second copy and the speculation of kf_raycast_volume_slab_cross_spec, bit for bit"""
    vol, _, _ = _volume("a104")
    inc = R.inc_for(vol[1], vol[2])
    g = _group("a104", R.RAGGED, LAYOUTS[1])
    key, cam, view, pose, near, far = next(c for c in _ragged_calls("a104") if c[2] == "corner-mixed")
    for m in g.members():
        a = [torch.empty((cam[1], cam[0]), dtype=torch.int64, device=DEV) for _ in range(4)]
        s = [torch.full((cam[1], cam[0], 3), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
        torch.cuda.synchronize()
        m.raycast_slab_cross_spec(pose, inc, near, far, a[0].data_ptr(), a[1].data_ptr(), s[0].data_ptr())
        form = m.raycast_form()
        m.view_slab_cross(False, pose, K.camera(*cam), inc, near, far, a[2].data_ptr(), a[3].data_ptr(), s[1].data_ptr())
        m.sync()
        assert m.raycast_form() == form
        assert torch.equal(a[0], a[2]) and torch.equal(a[1], a[3]) and torch.equal(a[0], a[1])
        assert torch.equal(s[0].view(torch.int32), s[1].view(torch.int32))
    g.close()


def test_sizes_that_stress_the_reduction_tails():
    """three cameras in a row on one group: ODD (7777 pixels: u64 tail 1, u32 tail 3), one pixel (no 16-byte unit at all) and BIG"""
    vol, _, ovol = _volume("a104")
    inc = R.inc_for(vol[1], vol[2])
    g = _group("a104", R.ODD, LAYOUTS[0])
    key, _, view, pose, near, far = next(c for c in _ragged_calls("a104") if c[2] == "front+z")
    assert R.ODD[0] * R.ODD[1] == 7777
    for cam in (R.ODD, ONE, BIG, ONE):
        if cam == ONE:
            ov, on, _ = O.raycast(ovol, False, pose, inc, O.Cam.make(*ONE), near, far)
            want = dict(v=ov, n=on, rgb=None)
            assert want["v"][0, 0, 3] == 1.0                   # aimed at the sphere through the shell's window
        else:
            want = _want("a104", key, cam)
        for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
            img, gv, gn = _render(g, mode, pose, cam, near, far)
            _check(key, mode, img, gv, gn, want, pose)
            assert g.view_size() == (cam[0], cam[1])
            assert int((img[..., 3] == 255).sum()) >= (1 if cam == ONE else R.min_hits(view, R.ODD))
    g.close()


def test_colour_group_views_equal_the_oracle():
    vol, _, _ = _volume("c64")
    g = _group("c64", R.ODD, [0, 32, 64])
    lone_total = 0
    for key, cam, view, pose, near, far in R.calls(vol):
        want = _want("c64", key, cam)
        for mode in MODES:                                      # (NORMALS and SHADED run with 3-word candidates on the colour group)
            img, gv, gn = _render(g, mode, pose, cam, near, far)
            _check(key, mode, img, gv, gn, want, pose)
        lone = (img[..., :3].astype(np.int32).sum(axis=-1) > 0) & (img[..., 3] == 0)      # (the COLOR picture) a colour and no normal
        assert np.array_equal(lone, (want["rgb"].astype(np.int32).sum(axis=-1) > 0) & (want["v"][..., 3] != 1.0)), key
        lone_total += int(lone.sum())
    assert lone_total >= 5, lone_total
    g.close()


def test_views_between_frames_change_nothing():
    """Scene S at 128^3 @ 3 m, VGA, cuts [0, 48, 128], 4 frames: once plain, once with a merged view after every frame"""
    cam, res, size, n = S.vga_camera(), 128, 3.0, 4
    frames = [S.render_depth_mm(S.trajectory_pose(k, size), cam, size) for k in range(n)]
    eye = R.look((1.2 * size, 0.4 * size, -0.4 * size), (-0.7, 0.1, 0.9)).astype(np.float32)
    runs = []
    for with_views in (False, True):
        g = G.Group.local(K.camera(*cam), res, size, [0, 48, 128])
        poses, results, forms = [], [], []
        for k in range(n):
            g.frame(frames[k], k)
            if with_views:
                g.render_view(K.VIEW_NORMALS if k & 1 else K.VIEW_SHADED, None if k & 1 else eye, K.camera(*R.RAGGED), P["depth_trunc_min"], 3.0 * size)
            r = g.track_result(check_lockstep=True)
            assert r[0] and r[2] == 0, (with_views, k)
            poses.append(r[1].copy()); results.append((r[0], r[2], r[3]))
            forms.append([m.raycast_form() for m in g.members()])
        if with_views:
            img = g.read_view()
            assert img.shape == (R.RAGGED[1], R.RAGGED[0], 4) and int((img[..., 3] == 255).sum()) >= 400
        maps = [[_bits(m.download_map(i, lv)).copy() for lv in range(3) for i in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS)] for m in g.members()]
        vols = [m.download_volume() for m in g.members()]
        runs.append(dict(poses=poses, results=results, forms=forms, maps=maps, vols=vols))
        g.close()
    a, b = runs
    assert a["results"] == b["results"] and a["forms"] == b["forms"], (a["forms"], b["forms"])
    assert a["forms"][-1][0]["calls"] == n
    for pa, pb in zip(a["poses"], b["poses"]):
        assert np.array_equal(_bits(pa), _bits(pb))
    for ma, mb in zip(a["maps"], b["maps"]):
        assert all(np.array_equal(x, y) for x, y in zip(ma, mb))
    for (ta, wa), (tb, wb) in zip(a["vols"], b["vols"]):
        assert np.array_equal(_bits(ta), _bits(tb)) and np.array_equal(wa, wb)


def _child(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k == "KF_STATS_CROSSCHECK"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_view_rccl_child.py"), mode], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "group view rccl ok" in r.stdout, "child %s exited with %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_rccl_all_world1_views_equal_the_local_group():
    _child("all1")


def test_rccl_rank_world1_views_equal_the_local_group():
    _child("rank1")


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason="needs two or more visible devices")
def test_rccl_views_over_every_visible_device():
    _child("alldev")


def test_cpp_slab_class_returns_the_groups_bytes():
    """HybKinectfuSlabs through the shim: 3 frames at 128^3, then renderView against Group.render_view on the borrowed group"""
    res, size, cam = 128, 3.0, S.vga_camera()
    trunc = 5 * size / res
    app = H.SlabsApp(res, size, cam, [0, 64, 128], sdf_trunc=trunc)
    try:
        for k in range(3):
            assert app.process_frame(S.render_depth_mm(S.trajectory_pose(k, size), cam, size), k)
        g = G.Group.borrow(app.group_handle(), K.camera(*cam), res, size)
        eye = R.look((1.1 * size, 0.45 * size, -0.3 * size), (-0.6, 0.05, 0.9)).astype(np.float32)
        for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
            for pose in (eye, None):
                got = app.render_view(mode, pose, R.RAGGED)
                g.render_view(mode, pose, K.camera(*R.RAGGED), P["depth_trunc_min"], P["depth_trunc_max"])
                assert np.array_equal(got, g.read_view()) and int((got[..., 3] == 255).sum()) >= 400, mode
        with pytest.raises(K.KfError):
            app.render_view(K.VIEW_COLOR, eye, R.RAGGED)             # the application has no colour plane
        g.close()
    finally:
        app.close()


def test_errors():
    vol, data, _ = _volume("a104")
    _, res, size, _, _ = vol
    inc = R.inc_for(res, size)
    g = _group("a104", R.ODD, LAYOUTS[0])
    key, cam, view, pose, near, far = _ragged_calls("a104")[0]
    kcam = K.camera(*cam)
    for fn in (g.read_view, g.view_size):                           # before any view
        with pytest.raises((G.GroupError, K.KfError), match="1002"):
            fn()
    assert g.view_device() is None
    img, _, _ = _render(g, K.VIEW_SHADED, pose, cam, near, far, maps=False)
    _check(key, K.VIEW_SHADED, img, None, None, _want("a104", key, cam), pose)
    zero = np.zeros((R.ODD[1], R.ODD[0]), np.uint16)
    refusals = [(-1, kcam, G.ERR_ARG), (3, kcam, G.ERR_ARG), (K.VIEW_COLOR, kcam, G.ERR_STATE), (K.VIEW_NORMALS, None, G.ERR_ARG)]
    refusals += [(K.VIEW_NORMALS, K.camera(c, r, *cam[2:]), G.ERR_ARG) for c, r in ((0, 152), (200, 0), (4097, 152), (200, 4097))]
    refusals += [(K.VIEW_NORMALS, K.camera(200, 152, 99.5, 75.5, fx, fy), G.ERR_ARG) for fx, fy in ((0.0, 164.0), (164.0, float("nan")))]
    refusals += [(K.VIEW_NORMALS, K.camera(200, 152, float("nan"), 75.5, 164.0, 164.0), G.ERR_ARG)]
    for k, (mode, c, code) in enumerate(refusals):
        with pytest.raises(G.GroupError) as e:
            g.render_view(mode, pose, c, near, far)
        assert e.value.status == code, (mode, code, e.value.status)
        assert g.view_size() == (cam[0], cam[1])                    # no refused call became "the last view"
        # the group stays usable: a view still renders, a frame still runs
        img, _, _ = _render(g, K.VIEW_NORMALS, pose, cam, near, far, maps=False)
        assert int((img[..., 3] == 255).sum()) >= R.min_hits(view, cam), (mode, code)
        g.frame(zero, k)
        g.track_result(check_lockstep=True)
    m0 = g.members()[0]
    buf = torch.zeros((cam[1], cam[0], 4), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(K.KfError, match="1001"):
        m0.view_from_rays(K.VIEW_COLOR, pose, kcam, buf.data_ptr(), buf.data_ptr(), 3)
    with pytest.raises(K.KfError, match="1002"):                    # colour forms need a colour plane
        m0.view_slab_cross(True, pose, kcam, inc, near, far, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    g.close()
    # a member whose halo is one brick thinner than the increment needs: ceil(7.5) + 2 = 10 layers, 8 stored
    thin = K.Context(K.camera(*R.ODD), res, size, P["volume_max_weight"], levels=3, slab=(0, 56), halo=8)
    ta = torch.zeros((cam[1], cam[0], 4), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(K.KfError, match="1001"):
        thin.view_slab_cross(False, pose, kcam, 7.5 * size / res, near, far, ta.data_ptr(), ta.data_ptr(), buf.data_ptr())
    thin.view_slab_cross(False, pose, kcam, inc, near, far, ta.data_ptr(), ta.data_ptr(), buf.data_ptr())      # (the scenarios' increment fits)
    thin.sync()
    thin.close()
