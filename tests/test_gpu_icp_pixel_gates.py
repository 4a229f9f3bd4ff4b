"""GPU: the ICP pixel phase gate by gate, on crafted maps whose 27 sums are exact in fp32 in any order (csrc/track.hip: icp_project, icp_finish, icp_accumulate).

The pixel phase is straight-line code: every gate is a boolean, all 2 x ICP_PX model-map gathers of a lane leave before the first wait, a pixel without a
correspondence reads model entry 0 and drops it, and the 27 fused multiply-adds of a pixel sit under ONE predicate.  What can go wrong with that form is a
gate that lets a pixel through (or the dummy read of entry 0 leaking into the sums), a rejected pixel's NaN / Inf reaching a sum, and a slot j of a lane
treated differently from the others.  So every case below is built for a pixel in slot j = 0, 1 and 2.

The maps, 96 x 64 (4 / 3 / 1 publishers: the smallest image with three pixels per lane at level 0 and one at levels 1 and 2):
  camera cx = 48, cy = 32, fx = fy = 64; identity pose; new vertex of pixel (u, v) = ((u - 48) / 64, (v - 32) / 64, 1): it projects onto (u, v) exactly;
  new normal = model normal = +-e_a, an axis chosen per 8 x 8 block (the pyramid's coarser normals stay unit axes and the maps track); model vertex =
  new vertex + small multiples of 1 / 64 along two axes.
Every row entry (q x n, n, n . (p - q)) is a multiple of 2^-6 and every product a multiple of 2^-12; the CPU side asserts that, and that the sum of the
absolute products of every one of the 27 sums stays below 2^24 quanta: every product and every partial sum is then exact in fp32 whatever the order, fused
or not.  So the comparison is for EQUALITY, against two references, neither of them the library: oracle_lib.icp_system (fp64 sums, cast to fp32) and the
closed form over the pixels a case accepts by construction (numpy, fp64).

Slots.  kf_cal_point_to_plane_solver_params (ctx.icp_system: k_icp_step, contiguous dealing) puts pixel i into slot (i % 1536) // 512; the tracking forms
deal 64-pixel chunks round robin over 4 workgroups and put pixel i into slot i // 2048 at level 0.  TARGET[j] lies in slot j under both rules.

The tracking forms (persistent loop against one launch per step, as tests/test_gpu_icp_pair_exchange.py compares them) run every case's maps too: same pose
bits, same final sums, same verdict."""
import numpy as np
import pytest

import oracle_lib as O
from hybkinectfu_amd import lib as K
from test_gpu_icp_fold_shapes import _publishers
from test_gpu_track_forms import _is

pytestmark = pytest.mark.gpu

COLS, ROWS = 96, 64
CAM = (COLS, ROWS, 48.0, 32.0, 64.0, 64.0)
Q = 64.0                                                         # row entries are multiples of 1 / Q
DIST, SIN = 0.25, 0.5                                            # the gates: |p - q| > 0.25 rejects, |n_t x n_g| > 0.5 rejects
SHAKE = (0.5, 0.5)                                               # camera-shake limits of the tracking runs (generous: the crafted motion is small)
EYE = np.eye(4, dtype=np.float32)
NPX = COLS * ROWS


def _slot_system(i):
    return (i % 1536) // 512


def _slot_loop(i):
    return i // 2048


# one pixel per slot, in slot j under both dealings; not on the principal axes (u != 48, v != 32) and away from the image edges
TARGET = [5 * COLS + 7, 2048 + 5 * COLS + 7, 4096 + 5 * COLS + 7]


def _base():
    """new vertices / normals and model vertices / normals, (ROWS, COLS, 4) f32 each, and the accepted mask (all true)"""
    u, v = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    nv = np.zeros((ROWS, COLS, 4), np.float32)
    nv[..., 0], nv[..., 1], nv[..., 2], nv[..., 3] = (u - 48) / Q, (v - 32) / Q, 1.0, 1.0
    axis = (u // 8 + 2 * (v // 8)) % 3                       # constant over 8 x 8 blocks: the pyramid's coarser normals stay unit axes, the maps trackable
    sign = np.where(((u // 16 + v // 8) % 2) == 0, 1.0, -1.0)
    nn = np.zeros((ROWS, COLS, 4), np.float32)
    for a in range(3):
        nn[..., a] = np.where(axis == a, sign, 0.0)
    mv = nv.copy()
    along, across = ((u % 3) - 1) / Q, ((v % 3) - 1) / Q      # the model sits up to 1 / 64 off along the normal and along the next axis
    for a in range(3):
        mv[..., a] += np.where(axis == a, along * sign, 0.0) + np.where((axis + 1) % 3 == a, across, 0.0)
    return nv, nn, mv, nn.copy(), np.ones((ROWS, COLS), bool)


def _flat(a):
    return a.reshape(NPX, -1) if a.ndim == 3 else a.reshape(NPX)


def _reject_own(maps, pixels):
    """knock pixels out by their own zero normal"""
    nv, nn, mv, mn, ok = maps
    _flat(nn)[pixels] = 0.0
    _flat(ok)[pixels] = False


def _case(name, j):
    """maps of one case for slot j; ok = the pixels it accepts by construction (each still corresponds to its own model pixel)"""
    maps = _base()
    nv, nn, mv, mn, ok = maps
    fnv, fnn, fmv, fmn, fok = (_flat(a) for a in maps)
    t = TARGET[j]
    assert _slot_system(t) == j and _slot_loop(t) == j
    if name == "base":
        pass
    elif name == "own_normal_zero":
        _reject_own(maps, [t])
    elif name in ("off_left", "off_right", "off_top", "off_bottom"):
        c, val = {"off_left": (0, -1.0), "off_right": (0, 1.0), "off_top": (1, -1.0), "off_bottom": (1, 1.0)}[name]
        fnv[t, c] = val                                          # px = -16 / 112, py = -32 / 96: clearly off the image
        fok[t] = False
    elif name == "z_zero":
        fnv[t, 2] = 0.0                                          # x, y != 0: the quotients are +-Inf, the conversion saturates, the bounds test rejects
        assert fnv[t, 0] != 0 and fnv[t, 1] != 0
        fok[t] = False
    elif name == "z_negative":
        fnv[t, 2] = -1.0                                         # projects onto the point-mirrored pixel (inside the image); the model there is 2 m away
        fok[t] = False
    elif name == "model_normal_zero":
        fmn[t] = 0.0
        fok[t] = False
    elif name == "dist_fails":
        fmv[t, :3] = fnv[t, :3] + np.float32([0.5, 0.0, 0.0])
        fok[t] = False
    elif name == "dist_equal_passes":
        fmv[t, :3] = fnv[t, :3] + np.float32([0.25, 0.0, 0.0])  # |p - q| == DIST exactly: `>` does not reject
    elif name == "angle_fails":
        fmn[t, :3] = np.roll(fmn[t, :3], 1)                      # the next axis: |n_t x n_g| = 1
        fok[t] = False
    elif name in ("nan_in_rejected_vertex", "inf_in_rejected_vertex"):
        bad = np.float32(np.nan if name.startswith("nan") else np.inf)
        _reject_own(maps, [t])
        fnv[t, :3] = [bad, -bad, bad]
    elif name in ("nan_in_rejected_model", "inf_in_rejected_model"):
        bad = np.float32(np.nan if name.startswith("nan") else np.inf)
        fmn[t] = 0.0                                             # the entry the pixel fetches: rejected for its zero normal, its vertex is poison
        fmv[t, :3] = [bad, bad, -bad]
        fok[t] = False
    elif name == "entry0_would_pass":
        _reject_own(maps, [t])                                   # reads entry 0 as a dummy ...
        fnv[t] = fmv[0]                                          # ... which lies exactly where this pixel is (distance 0; its own normal is zero: sine 0)
        assert not np.all(fmn[0] == 0)
    elif name == "whole_lane_rejected":
        t0 = TARGET[0]                                           # the three pixels of one lane, under both dealings
        _reject_own(maps, [t0, t0 + 512, t0 + 1024, t0 + 2048, t0 + 4096])
    elif name == "wave_only_one_slot":                           # wave 0 of workgroup 0: only its pixels of slot j keep accepted lanes, under both dealings
        sysform = [c for c in (0, 512, 1024) if _slot_system(c) != j]
        loopform = [c for c in (0, 2048, 4096) if _slot_loop(c) != j]
        for c in sorted(set(sysform + loopform)):
            _reject_own(maps, list(range(c, c + 64)))
    else:
        raise KeyError(name)
    return maps


CASES = ["base", "own_normal_zero", "off_left", "off_right", "off_top", "off_bottom", "z_zero", "z_negative", "model_normal_zero", "dist_fails",
         "dist_equal_passes", "angle_fails", "nan_in_rejected_vertex", "inf_in_rejected_vertex", "nan_in_rejected_model", "inf_in_rejected_model",
         "entry0_would_pass", "whole_lane_rejected", "wave_only_one_slot"]


def _closed_form(maps):
    """the 27 sums over the accepted pixels, fp64; asserts the exactness conditions (multiples of 2^-6, fewer than 2^24 quanta of 2^-12 per sum)"""
    nv, nn, mv, mn, ok = maps
    m = _flat(ok)
    q, p, n = (_flat(a)[m, :3].astype(np.float64) for a in (nv, mv, mn))
    row = np.concatenate([np.cross(q, n), n, np.sum(n * (p - q), axis=1, keepdims=True)], axis=1)
    assert np.all(np.isfinite(row)) and np.array_equal(row * Q, np.round(row * Q))
    sums, s = np.zeros(27), 0
    for r in range(6):
        for c in range(r, 7):
            prod = row[:, r] * row[:, c]
            assert np.sum(np.abs(prod)) * Q * Q < 2.0 ** 24
            sums[s] = np.sum(prod)
            s += 1
    return sums


@pytest.fixture
def ctx():                                                       # per test: conftest closes every live context after each test
    assert _publishers(COLS, ROWS) == [4, 3, 1]
    c = K.Context(K.camera(*CAM), 32, 3.0, levels=3)
    yield c
    c.close()


def _upload(ctx, maps):
    nv, nn, mv, mn, _ = maps
    ctx.upload_map(K.MAP_NEW_VERTICES, 0, nv)
    ctx.upload_map(K.MAP_NEW_NORMALS, 0, nn)
    ctx.upload_map(K.MAP_MODEL_VERTICES, 0, mv)
    ctx.upload_map(K.MAP_MODEL_NORMALS, 0, mn)


@pytest.mark.parametrize("j", [0, 1, 2])
@pytest.mark.parametrize("name", CASES)
def test_sums_equal_the_oracle_and_the_closed_form(ctx, name, j):
    maps = _case(name, j)
    nv, nn, mv, mn, ok = maps
    want = _closed_form(maps)
    sd, _, valid = O.icp_system(nv, nn, mv, mn, O.Cam.make(*CAM), EYE, EYE, DIST, SIN)
    assert valid == int(ok.sum())                               # the two references agree on who is accepted ...
    assert np.array_equal(sd, want)                             # ... and on the sums (both fp64, both exact)
    _upload(ctx, maps)
    g = ctx.icp_system(0, EYE, EYE, ctx.cam, DIST, SIN)
    print(name, j, "accepted", valid, "max |gpu - oracle|", np.max(np.abs(g.astype(np.float64) - sd)))
    assert np.array_equal(g, sd.astype(np.float32)), (name, j, g, sd)
    assert np.array_equal(g, want.astype(np.float32))


def _track(ctx, maps):
    _upload(ctx, maps)
    ctx.set_pose(EYE)
    ctx.icp_track(1, DIST, SIN, *SHAKE)
    ok, p, status, iters = ctx.track_result()
    return ok, p, status, iters, ctx.last_form, ctx.read_solver_params()


def test_persistent_loop_equals_the_per_step_form_on_every_case(ctx):
    cases = [(name, j) for name in CASES for j in (0, 1, 2)]
    loop = [_track(ctx, _case(name, j)) for name, j in cases]
    other = K.Context(K.camera(*CAM), 32, 3.0, levels=3)            # a second live context: one launch per step
    step = [_track(ctx, _case(name, j)) for name, j in cases]
    other.close()
    for (name, j), (ok1, p1, st1, it1, form1, sums1), (ok2, p2, st2, it2, form2, sums2) in zip(cases, loop, step):
        assert _is(form1, 1) and _is(form2, 2), (name, j, form1, form2)
        assert ok1 and ok2 and st1 == st2 == 0 and it1 == it2 == 19, (name, j, ok1, ok2, st1, st2, it1, it2)
        assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)), (name, j)           # same pose bits
        assert np.array_equal(sums1.view(np.uint32), sums2.view(np.uint32)), (name, j)     # same final 27 sums
        assert np.all(np.isfinite(p1)) and np.all(np.isfinite(sums1)), (name, j)           # no poison reached a sum
