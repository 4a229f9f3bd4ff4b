"""GPU: the two forms of the bilateral filter give the same bits, and the streamed sequence without a far gate equals the plain one and the oracle.

The gate + bilateral filter (DataPreprocesser.cu) comes in two forms (bilateral_tile.h): FAST keeps an invalid pixel in the LDS tile as a huge sentinel
whose tap weight underflows to zero; the other tests validity per tap.  kf_bilateral_args picks the sentinel form for every sane parameter set -- not
when trunc_max >= 1e15 (no far gate: a valid depth could reach the sentinel) or sigma_depth is extreme.  The rest of the suite runs with the stock far
gate only, so k_gate_bilateral<4, false>, k_raycast_prefetch<false> and the ICP loop's rider kf_bilateral_tile<4, false> ran in no test."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import default_forms

import filter_stream_child as FS
import oracle_lib as O
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

pytestmark = pytest.mark.gpu
P = S.STOCK
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("cam", [(200, 152, 99.5, 75.5, 164.0, 164.0), S.vga_camera()])
def test_sentinel_and_per_tap_filters_agree(cam, noise):
    """no depth reaches either gate (1e14 m: the sentinel form; +inf: the per-tap form), so both must give the same raw, gated and filtered depth,
    vertices and normals -- noise puts holes next to valid pixels and depth steps beyond 5 sigma (the filter's early return)"""
    size = 3.0
    ctx = K.Context(K.camera(*cam), 32, size, levels=3)
    for k in (0, 9, 23):
        mm = S.render_depth_mm(S.trajectory_pose(k, size), cam, size)
        if noise:
            mm = S.add_sensor_noise(mm[None], first_frame=k)[0]
        assert int((mm == 0).sum()) > (100 if noise else -1)
        ctx.upload_depth_mm(mm)
        got = []
        for tmax in (1e14, float("inf")):
            ctx.preprocess(P["depth_trunc_min"], tmax, P["filter_sigma_pixel"], P["filter_sigma_depth"])
            got.append([bits(ctx.download_map(m)) for m in FS.MAPS[:5]])
        for a, b, m in zip(got[0], got[1], FS.MAPS[:5]):
            assert np.array_equal(a, b), (k, noise, m)
    ctx.close()


def test_stream_without_far_gate_every_mode_equals_plain_and_the_oracle(tmp_path):
    runs = {mode: FS.run(mode) for mode in ("plain", "prefetch", "prefetch-per-step")}
    env = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k in ("KF_STATS_CROSSCHECK", "KF_ORACLE_SO", "KF_LIB")}
    env["KF_PREFETCH_FUSED"] = "0"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = str(tmp_path / "side.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "filter_stream_child.py"), out, "prefetch"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    runs["side-stream"] = dict(poses=z["poses"], maps=[z["map%d" % i] for i in range(len(FS.MAPS))], tsdf=z["tsdf"], weight=z["weight"],
                               track_forms=z["track_forms"], rc_forms=z["rc_forms"])
    plain = runs["plain"]
    for mode, got in runs.items():
        assert np.array_equal(got["poses"].view(np.uint32), plain["poses"].view(np.uint32)), mode
        for a, b, m in zip(got["maps"], plain["maps"], FS.MAPS):
            assert np.array_equal(bits(a), bits(b)), (mode, m)
        assert np.array_equal(bits(got["tsdf"]), bits(plain["tsdf"])) and np.array_equal(bits(got["weight"]), bits(plain["weight"])), mode
        # every launch with a rider took the per-tap form (no far gate)
        rc = got["rc_forms"]
        assert not (rc[:, 1] != 0).any(), (mode, rc)
    # which launch carried the filter: the raycast only when the tracker ran per step, or in the side-stream form never
    kinds = {mode: set(int(k) for k in got["rc_forms"][:-1, 0]) for mode, got in runs.items()}
    assert kinds["plain"] == {K.RC_PLAIN} and kinds["side-stream"] == {K.RC_PLAIN}, kinds
    if default_forms():
        # (frame 0 has no tracking launch for the filter to ride in)
        assert K.RC_BEHIND in kinds["prefetch"] <= {K.RC_BEHIND, K.RC_FILTER} and kinds["prefetch-per-step"] == {K.RC_FILTER}, kinds
        assert 1 in runs["prefetch"]["track_forms"] and 2 in runs["prefetch-per-step"]["track_forms"] and 1 not in runs["prefetch-per-step"]["track_forms"]
    assert int(runs["plain"]["rc_forms"][-1, 0]) == K.RC_PLAIN and all(int(g["rc_forms"][-1, 0]) == K.RC_PLAIN for g in runs.values())
    # plain against the oracle, last frame: raw and gated depth exact, filtered within 2e-6 relative (device __expf), vertices and normals exact
    # from the device's own filtered map
    mm = FS.frames()[-1]
    ocam = O.Cam.make(*FS.CAM)
    d = O.depth_mm_to_m(mm)
    tr = O.trunc_depth(d, P["depth_trunc_min"], float("inf"))
    fl = O.bilateral(tr, P["filter_sigma_pixel"], P["filter_sigma_depth"])
    raw, gated, g_fl, gv, gn = plain["maps"][:5]
    assert np.array_equal(bits(raw), bits(d)) and np.array_equal(bits(gated), bits(tr))
    assert np.allclose(g_fl, fl, rtol=2e-6, atol=0) and np.array_equal(g_fl == 0, fl == 0)
    v2 = O.depth_to_vertices(g_fl, ocam)
    assert np.array_equal(bits(gv), bits(v2)) and np.array_equal(bits(gn), bits(O.vertices_to_normals(v2)))
