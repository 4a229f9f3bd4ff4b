"""GPU: viewer frames -- kf_render_view (a free viewpoint marched through the volume, display bytes out) and kf_view_model_maps (the tracking
camera's view from the model maps) against the CPU oracle's raycast and the numpy restatement of the byte formulas (view_expect.py).

The volumes and viewpoints are those of raycast_scenarios.py.  The float4 maps a view leaves on request must equal the oracle's bit for bit, and
the picture must equal view_expect applied to those maps byte for byte.  A view is a bystander: model maps, raycast colours, the raycast form's
record, a pending prefetch, poses and the fused volume are the same with and without it."""
import numpy as np
import pytest
import torch

import raycast_scenarios as R
import view_expect as V
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import pipeline as PL
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = R.P
DEV = torch.device("cuda", 0)
BIG = (416, 304, 207.5, 151.5, 340.0, 340.0)           # larger than the contexts' cameras both ways: 13 x 19 ray tiles
SPARSE = ("far", "axes-x", "axes-y") + R.ZERO_HIT_VIEWS
MODES = (K.VIEW_NORMALS, K.VIEW_SHADED, K.VIEW_COLOR)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _volume(vid):
    vol = next(v for v in R.VOLUMES if v[0] == vid)
    data = R.volume_data(vol)
    return vol, data, R.oracle_volume(vol, data)


def _context(vol, data, cam, **kw):
    _, res, size, color, _ = vol
    ctx = K.Context(K.camera(*cam), res, size, P["volume_max_weight"], levels=3, has_color=color, **kw)
    s0, s1 = ctx.stored
    ctx.upload_volume(data[0][s0:s1], data[1][s0:s1], data[2][s0:s1] if color else None)
    return ctx


def _render(ctx, mode, pose, cam, inc, near, far, maps=True):
    """one kf_render_view; returns (image, v, n) -- the maps from caller-owned buffers that start as NaN, so every pixel must be written"""
    dv = dn = None
    if maps:
        dv = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
        dn = torch.full((cam[1], cam[0], 4), float("nan"), dtype=torch.float32, device=DEV)
    ctx.render_view(mode, pose, K.camera(*cam), inc, near, far, dv.data_ptr() if maps else None, dn.data_ptr() if maps else None)
    img = ctx.read_view()
    assert ctx.view_size() == (cam[0], cam[1]) and img.shape == (cam[1], cam[0], 4) and ctx.view_device()
    return img, (dv.cpu().numpy() if maps else None), (dn.cpu().numpy() if maps else None)


def _check_view(key, mode, img, gv, gn, want, pose):
    if gv is not None:
        assert np.array_equal(_bits(gv), _bits(want["v"])), (key, mode)
        assert np.array_equal(_bits(gn), _bits(want["n"])), (key, mode)
    exp = V.view_bytes(mode, want["v"], want["n"], rgb=want["rgb"], eye=pose[:3, 3])
    assert np.array_equal(img, exp), (key, mode, int((img != exp).any(axis=-1).sum()))


def test_free_viewpoint_equals_the_oracle():
    """a104 from every side: the context is created with the ODD camera and the views are rendered with RAGGED -- another size, no multiple of the ray tile"""
    vol, data, ovol = _volume("a104")
    inc = R.inc_for(vol[1], vol[2])
    ctx = _context(vol, data, R.ODD)
    calls = [c for c in R.calls(vol) if c[1] == R.RAGGED]
    assert len(calls) == len(R.views(vol[2], vol[1]))
    for call in calls:
        key, cam, view, pose, near, far = call
        want = R.oracle_maps(vol, ovol, call)
        hit = want["v"][..., 3] == 1.0
        for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
            img, gv, gn = _render(ctx, mode, pose, cam, inc, near, far)
            _check_view(key, mode, img, gv, gn, want, pose)
            # (the picture is not one flat value: half of what the oracle's maps give on the CPU, tests/test_view_abi_cpu.py)
            n_hit = int((img[..., 3] == 255).sum())
            assert n_hit == int(hit.sum()) and R.hits(gn) >= R.min_hits(view, cam), (key, n_hit)
            if view in R.ZERO_HIT_VIEWS:
                assert n_hit == 0 and np.all(img[..., 3] == 0) and np.all(img[..., :3] == (127 if mode == K.VIEW_NORMALS else 0)), key
            if view not in SPARSE:
                assert n_hit >= 2300, (key, n_hit)
                if mode == K.VIEW_SHADED:
                    assert len(np.unique(img[hit][:, 0])) >= 100, key
                else:
                    assert len(np.unique(img[hit][:, :3], axis=0)) >= 375, key
    # a camera larger than the context's in both directions, and views without the optional maps
    for name in ("front+z", "corner-mixed", "inside-diag"):
        call = next(c for c in calls if c[2] == name)
        big = (call[0] + "/big", BIG) + call[2:]
        want = R.oracle_maps(vol, ovol, big)
        for mode, maps in ((K.VIEW_NORMALS, True), (K.VIEW_SHADED, False)):
            img, gv, gn = _render(ctx, mode, big[3], BIG, inc, big[4], big[5], maps=maps)
            _check_view(big[0], mode, img, gv, gn, want, big[3])
            assert int((img[..., 3] == 255).sum()) >= 4 * 2300, big[0]
    # smaller again: the image buffer is reused, the size follows the last view
    img, _, _ = _render(ctx, K.VIEW_SHADED, calls[0][3], R.ODD, inc, calls[0][4], calls[0][5], maps=False)
    want = R.oracle_maps(vol, ovol, (calls[0][0], R.ODD) + calls[0][2:])
    _check_view("odd", K.VIEW_SHADED, img, None, None, want, calls[0][3])
    ctx.close()


def test_free_viewpoint_colour_equals_the_oracle():
    vol, data, ovol = _volume("c64")
    inc = R.inc_for(vol[1], vol[2])
    ctx = _context(vol, data, R.ODD)
    lone_total = 0
    for call in R.calls(vol):
        key, cam, view, pose, near, far = call
        want = R.oracle_maps(vol, ovol, call)
        for mode in MODES:
            img, gv, gn = _render(ctx, mode, pose, cam, inc, near, far)
            _check_view(key, mode, img, gv, gn, want, pose)
        lone = (img[..., :3].astype(np.int32).sum(axis=-1) > 0) & (img[..., 3] == 0)      # (the COLOR picture) a colour and no normal
        assert np.array_equal(lone, (want["rgb"].astype(np.int32).sum(axis=-1) > 0) & (want["v"][..., 3] != 1.0)), key
        lone_total += int(lone.sum())
        assert len(np.unique(img[img[..., 3] == 255][:, :3], axis=0)) >= 100, key
    assert lone_total >= 5, lone_total
    ctx.close()


def _tracking_state(ctx, color):
    out = {}
    for lv in range(3):
        out["v%d" % lv] = _bits(ctx.download_map(K.MAP_MODEL_VERTICES, lv)).copy()
        out["n%d" % lv] = _bits(ctx.download_map(K.MAP_MODEL_NORMALS, lv)).copy()
    if color:
        out["rgb"] = ctx.download_map(K.MAP_RAYCAST_RGB).copy()
    return out, ctx.raycast_form()


@pytest.mark.parametrize("vid", ["fused", "c64"])
def test_a_view_leaves_the_raycast_outputs_alone(vid):
    """after kf_raycast_volume: the model maps at all three levels, KF_MAP_RAYCAST_RGB and kf_get_raycast_form's record, `calls` included, are the
    same before and after a kf_render_view from another pose with another camera"""
    vol, data, ovol = _volume(vid)
    _, res, size, color, _ = vol
    inc = R.inc_for(res, size)
    calls = [c for c in R.calls(vol) if c[1] == R.RAGGED]
    first, other = next(c for c in calls if c[2] == "front+z"), next(c for c in calls if c[2] == "corner-mixed")
    if vid == "fused":
        ctx = K.Context(K.camera(*R.RAGGED), res, size, P["volume_max_weight"], levels=3)
        R.fuse_gpu(ctx)
    else:
        ctx = _context(vol, data, R.RAGGED)
    ctx.raycast(first[3], inc, first[4], first[5], has_color=color)
    before, form_before = _tracking_state(ctx, color)
    assert form_before["calls"] == 1 and R.hits(before["n0"].view(np.float32)) >= R.min_hits("front+z", R.RAGGED)
    want = R.oracle_maps(vol, ovol, (other[0], R.ODD) + other[2:])
    for mode in MODES if color else MODES[:2]:
        img, gv, gn = _render(ctx, mode, other[3], R.ODD, inc, other[4], other[5])
        _check_view(other[0], mode, img, gv, gn, want, other[3])
        after, form_after = _tracking_state(ctx, color)
        assert form_after == form_before, (form_before, form_after)
        for k in before:
            assert np.array_equal(before[k], after[k]), (mode, k)
    ctx.close()


def test_views_in_the_streamed_pipeline_change_nothing():
    """SingleGpuPipeline over 8 frames of Scene S at 128^3, frames in HBM, the next frame's front end riding in each frame's launches: a view enqueued
    after every frame leaves pose bits, launch forms, the cull tails' counts and the fused volume as they are without it"""
    cam, res, size, n = S.vga_camera(), 128, 3.0, 8
    frames, _ = S.make_stream(n, cam, size)
    dev = torch.from_numpy(frames.astype(np.int16)).cuda()
    fb = cam[0] * cam[1] * 2
    eye = R.look((1.2 * size, 0.4 * size, -0.4 * size), (-0.7, 0.1, 0.9)).astype(np.float32)
    runs = []
    for with_views in (False, True):
        pipe = PL.SingleGpuPipeline(K.camera(*cam), res, size, dict(trunc_max=P["depth_trunc_max"], integ_dist=P["integrate_depth_trunc"]))
        poses, forms, rc = [], [], []
        for k in range(n):
            pipe.process_frame_device(dev.data_ptr() + k * fb, k, dev.data_ptr() + ((k + 1) % n) * fb)
            rc.append(pipe.ctx.raycast_form())
            if with_views:
                pipe.ctx.render_view(K.VIEW_SHADED if k & 1 else K.VIEW_NORMALS, eye if k % 3 else None, K.camera(*R.RAGGED), pipe.inc,
                                     P["depth_trunc_min"], 3.0 * size)
                assert pipe.ctx.raycast_form() == rc[-1]
            ok, pose, status, _ = pipe.track_result()
            assert ok and status == 0, (with_views, k)
            poses.append(pose.copy()); forms.append(pipe.ctx.last_form)
        if with_views:
            img = pipe.ctx.read_view()
            assert img.shape == (R.RAGGED[1], R.RAGGED[0], 4) and int((img[..., 3] == 255).sum()) >= 400
        st = pipe.stats()
        runs.append(dict(poses=poses, forms=forms, rc=rc, tails=pipe.ctx.cull_tail_counts(), vol=pipe.ctx.download_volume(),
                         upd=st["updated_total"], fused=st["frames_fused"], lost=st["frames_lost"]))
        pipe.close()
    a, b = runs
    assert a["forms"] == b["forms"] and a["rc"] == b["rc"] and a["tails"] == b["tails"], (a["forms"], b["forms"], a["tails"], b["tails"])
    assert (a["upd"], a["fused"], a["lost"]) == (b["upd"], b["fused"], b["lost"]) and a["fused"] == n
    for pa, pb in zip(a["poses"], b["poses"]):
        assert np.array_equal(_bits(pa), _bits(pb))
    assert np.array_equal(_bits(a["vol"][0]), _bits(b["vol"][0])) and np.array_equal(a["vol"][1], b["vol"][1])


def test_view_model_maps_equals_the_formulas_on_the_model_maps():
    vol, data, ovol = _volume("c64")
    inc = R.inc_for(vol[1], vol[2])
    ctx = _context(vol, data, R.RAGGED)
    for call in [c for c in R.calls(vol) if c[2] in ("front+z", "corner-mixed", "roll30")]:
        key, cam, view, pose, near, far = call
        ctx.set_pose(pose)
        ctx.raycast(None, inc, near, far, has_color=True)
        mv, mn, rgb = ctx.download_map(K.MAP_MODEL_VERTICES), ctx.download_map(K.MAP_MODEL_NORMALS), ctx.download_map(K.MAP_RAYCAST_RGB)
        want = R.oracle_maps(vol, ovol, call)
        assert np.array_equal(_bits(mv), _bits(want["v"])) and np.array_equal(rgb, want["rgb"]), key
        for mode in MODES:
            ctx.view_model_maps(mode)
            img = ctx.read_view()
            exp = V.view_bytes(mode, mv, mn, rgb=rgb, eye=pose[:3, 3])
            assert np.array_equal(img, exp), (key, mode)
            # ... which is what the free viewpoint gives for the tracking camera and pose
            img2, _, _ = _render(ctx, mode, None, cam, inc, near, far, maps=False)
            assert np.array_equal(img2, exp), (key, mode)
        assert int((exp[..., 3] == 255).sum()) >= R.min_hits(view, cam)
    ctx.close()


def _merge(slabs, cam, pose, inc, near, far):
    """the slab protocol of SlabPipeline on contexts that share one device (what tests/test_gpu_raycast_sides.py runs)"""
    tas, owns, specs = [], [], []
    for c in slabs:
        ta, own = torch.empty((cam[1], cam[0]), dtype=torch.int64, device=DEV), torch.empty((cam[1], cam[0]), dtype=torch.int64, device=DEV)
        spec = torch.empty((cam[1], cam[0], 3), dtype=torch.float32, device=DEV)
        c.raycast_slab_cross_spec(pose, inc, near, far, ta.data_ptr(), own.data_ptr(), spec.data_ptr())
        tas.append(ta); owns.append(own); specs.append(spec)
    for c in slabs:
        c.sync()
    ta_min = torch.stack(tas).min(dim=0).values.contiguous()
    acc = torch.zeros((cam[1], cam[0], 3), dtype=torch.int32, device=DEV)
    for c, own, spec in zip(slabs, owns, specs):
        cand = torch.empty((cam[1], cam[0], 3), dtype=torch.float32, device=DEV)
        c.slab_ray_normals_spec(pose, inc, near, far, ta_min.data_ptr(), own.data_ptr(), spec.data_ptr(), cand.data_ptr())
        c.sync()
        acc += cand.view(torch.int32)
    rays = acc.view(torch.float32).contiguous()
    for c in slabs:
        c.set_model_maps_rays(pose, ta_min.data_ptr(), rays.data_ptr())
        c.sync()


def test_view_model_maps_on_slab_members_shows_the_whole_volume():
    vol, data, ovol = _volume("a104")
    _, res, size, _, _ = vol
    inc = R.inc_for(res, size)
    halo = PL.slab_halo_layers(res, size, inc)
    slabs = [_context(vol, data, R.RAGGED, slab=r, halo=halo) for r in PL.slab_ranges(res, 2)]
    for call in [c for c in R.calls(vol) if c[1] == R.RAGGED and c[2] in ("front+z", "back-z", "corner-mixed")]:
        key, cam, view, pose, near, far = call
        _merge(slabs, cam, pose, inc, near, far)
        want = R.oracle_maps(vol, ovol, call)
        for c in slabs:
            c.set_pose(pose)
            for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
                c.view_model_maps(mode)
                img = c.read_view()
                exp = V.view_bytes(mode, want["v"], want["n"], eye=pose[:3, 3])
                assert np.array_equal(img, exp), (key, mode, c.owned)
                assert int((img[..., 3] == 255).sum()) >= 2300, key
            # a member sees only its own layers: no free viewpoint from it
            with pytest.raises(K.KfError, match="1002"):
                c.render_view(K.VIEW_NORMALS, pose, K.camera(*cam), inc, near, far)
    for c in slabs:
        c.close()


def test_host_classes_return_the_contexts_bytes():
    res, size, cam = 128, 3.0, S.vga_camera()
    trunc = 5 * size / res
    app = H.App(res, size, cam, sdf_trunc=trunc)
    for k in range(3):
        assert app.process_frame(S.render_depth_mm(S.trajectory_pose(k, size), cam, size), k)
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*cam), res, size)
    inc = float(np.float32(0.7) * np.float32(trunc))           # hkf_app_init: 0.7f * sdf_trunc
    eye = R.look((1.1 * size, 0.45 * size, -0.3 * size), (-0.6, 0.05, 0.9)).astype(np.float32)
    for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
        for pose in (eye, None):
            got = app.render_view(mode, pose, R.RAGGED)
            ctx.render_view(mode, pose, K.camera(*R.RAGGED), inc, P["depth_trunc_min"], P["depth_trunc_max"])
            exp = ctx.read_view()
            assert np.array_equal(got, exp) and int((got[..., 3] == 255).sum()) >= 400, mode
        got = app.view_model_maps(mode)
        ctx.view_model_maps(mode)
        exp = ctx.read_view()
        mv, mn = ctx.download_map(K.MAP_MODEL_VERTICES), ctx.download_map(K.MAP_MODEL_NORMALS)
        assert np.array_equal(got, exp) and np.array_equal(got, V.view_bytes(mode, mv, mn, eye=app.pose()[1][:3, 3])), mode
        assert int((got[..., 3] == 255).sum()) >= 4000
    with pytest.raises(K.KfError):
        app.render_view(K.VIEW_COLOR, eye, R.RAGGED)             # the application has no colour plane
    ctx.close()
    app.close()


def test_errors():
    vol, data, _ = _volume("a104")
    inc = R.inc_for(vol[1], vol[2])
    ctx = _context(vol, data, R.ODD)
    with pytest.raises(K.KfError, match="1002"):
        ctx.read_view()                                          # before any view
    with pytest.raises(K.KfError, match="1002"):
        ctx.view_size()
    assert ctx.view_device() is None
    pose = R.views(vol[2], vol[1])[0][1].astype(np.float32)
    with pytest.raises(K.KfError, match="1002"):
        ctx.render_view(K.VIEW_COLOR, pose, K.camera(*R.RAGGED), inc, R.NEAR, R.FAR)      # no colour plane
    with pytest.raises(K.KfError, match="1002"):
        ctx.view_model_maps(K.VIEW_COLOR)
    for mode in (-1, 3):
        with pytest.raises(K.KfError, match="1001"):
            ctx.render_view(mode, pose, K.camera(*R.RAGGED), inc, R.NEAR, R.FAR)
        with pytest.raises(K.KfError, match="1001"):
            ctx.view_model_maps(mode)
    with pytest.raises(K.KfError, match="1001"):
        ctx.render_view(K.VIEW_NORMALS, pose, K.camera(0, 152, *R.RAGGED[2:]), inc, R.NEAR, R.FAR)
    with pytest.raises(K.KfError, match="1002"):
        ctx.read_view()                                          # none of the refused calls became "the last view"
    ctx.render_view(K.VIEW_NORMALS, pose, K.camera(*R.RAGGED), inc, R.NEAR, R.FAR)
    assert ctx.read_view().shape == (R.RAGGED[1], R.RAGGED[0], 4)
    half = K.Context(K.camera(*R.ODD), vol[1], vol[2], P["volume_max_weight"], levels=3, slab=(0, 56), halo=16)
    with pytest.raises(K.KfError, match="1002"):
        half.render_view(K.VIEW_NORMALS, pose, K.camera(*R.RAGGED), inc, R.NEAR, R.FAR)   # a z-slab context
    half.close()
    ctx.close()
