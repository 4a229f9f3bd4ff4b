"""GPU: relocalising a frame in the map.  kf_map_score_poses scores candidate camera poses of one point set against the map in integers, kf_map_pose_sums
forms the Gauss-Newton sums of several poses in one launch, kf_map_refine_poses runs kf_align_brick_store's loop over them.  The yardstick is
tests/map_reloc_expect.py (the rule of include/hybkf.h restated in numpy over map_query_expect.np_sample), held against closed forms by
tests/test_map_reloc_cpu.py, which also records the refinement's bound: np_refine recovers every start of OFFSETS to 0.1152 voxels at the points, the bound
here is four times that, 0.4608 voxels.  Shapes, stream and helpers are those of test_gpu_map_query.py.  Scores are compared as bytes; the sums by the bound
of test_gpu_map_align.py, count * 2^-52 * sum |term| around the correctly rounded sum, and bit for bit between runs and contexts."""
import ctypes as C
import functools

import numpy as np
import pytest

import map_query_expect as E
import map_reloc_expect as R
import test_gpu_map_query as Q
import test_gpu_shift as G
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ARG, STATE = 1001, 1002
CASES = Q.CASES
FIELDS = ("n_obs", "n_in", "n_behind", "n_free", "sum_q")


def same_scores(got, want, what):
    assert got.dtype == want.dtype == K.POSE_SCORE_DTYPE and got.tobytes() == want.tobytes(), (what, [int(np.count_nonzero(got[k] != want[k])) for k in FIELDS])


def moved_poses(poses, db):
    return np.stack([R.moved_pose(P, db) for P in poses])


@functools.lru_cache(maxsize=None)
def cuboid_scores():
    return R.np_score(R.cuboid_index(), R.scene()[1], R.score_poses(), R.BAND)


@functools.lru_cache(maxsize=None)
def many_points():
    """16 500 points: the scene's, then copies moved by multiples of 2^-6 along the camera's x and y, with one point in 97 not a number"""
    pts = R.scene()[1]
    n = 16500
    reps = -(-n // len(pts))
    out = np.concatenate([pts + f32(2.0 ** -6) * np.array([r % 7, r // 7, 0], f32) for r in range(reps)])[:n].copy()
    out[50::97, 1] = np.nan
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def many_samples():
    """per pose of score_poses() and point of the first 4 097 of many_points(): (tsdf, observed) of the yardstick's sample"""
    pts = many_points()[:4097]
    t, o = [], []
    for P in R.score_poses():
        s = E.np_sample(R.cuboid_index(), R.positions(pts, P))
        t.append(s["tsdf"]); o.append(s["observed"])
    return np.stack(t), np.stack(o)


# ---- 1. the analytic map, at the origin and at far keys, through store and window, both forms -------------------------------------------------------------
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("res,color", CASES)
def test_scores_on_the_analytic_map(res, color, far):
    db = E.FAR if far else (0, 0, 0)
    pts, poses, want = R.scene()[1], R.score_poses(), cuboid_scores()
    ctx = Q.store_only_ctx(res, color, E.shifted(R.cuboid_map(), db))
    q = moved_poses(poses, db)
    q[-1] = poses[-1]                                             # (the pose beyond the key range stays where it is)
    got = ctx.map_score_poses(pts, q, R.BAND)
    same_scores(got, want, ("store", far))
    assert got["n_obs"][0] == len(pts) == got["n_in"][0] and min(got["n_in"].sum(), got["n_behind"].sum(), got["n_free"].sum()) >= 32
    assert np.all(got["n_obs"][-2:] == 0)
    if not far:                                                   # the same map seen through the window: placed over it, the window answers
        ctx.place_window(0, 0, 0)
        assert ctx.volume_origin() == (0, 0, 0)
        same_scores(ctx.map_score_poses(pts, q, R.BAND), want, "window")
    ctx.close()


def test_device_form():
    import torch
    pts, poses, want = R.scene()[1], R.score_poses(), cuboid_scores()
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    dev = torch.device("cuda")
    d_pts, d_poses = torch.from_numpy(np.array(pts)).to(dev), torch.from_numpy(np.array(poses)).to(dev)
    d_out = torch.full((len(poses) * 24,), 7, dtype=torch.uint8, device=dev)      # (the call zeroes it)
    torch.cuda.synchronize()
    ctx.map_score_poses_device(len(pts), d_pts.data_ptr(), len(poses), d_poses.data_ptr(), R.BAND, d_out.data_ptr())
    ctx.sync()
    same_scores(d_out.cpu().numpy().view(K.POSE_SCORE_DTYPE), want, "device")
    same_scores(ctx.map_score_poses(pts, poses, R.BAND), want, "host")
    ctx.close()


# ---- 2. the fused map, partly in the window, partly in the store ---------------------------------------------------------------------------------------------
def frame_queries(ctx):
    """points: the hits of the pose's camera rays (every 4th) through the map, in the camera frame, voxels; poses: the pose in world voxels and 23 around it, up
    to 10 voxels and 6 degrees off -- the surface reaches from the window into the store, and so do the points"""
    cell = f32(ctx.size) / f32(ctx.res)
    pose = np.asarray(G.pose_of(ctx), f64)
    o, d = Q.camera_rays(pose, G.CAM, cell, ctx.volume_origin())
    r = ctx.map_cast_rays(o, d, f32(0.4) / cell, f32(3.0) / cell, f32(3.5))
    hit = r["status"] == K.RAY_HIT
    world = o[hit] + (r["t"][hit][:, None] * d[hit]).astype(f64)
    Pv = np.concatenate([pose[:3, :3], (pose[:3, 3] / float(cell) + np.array(ctx.volume_origin(), f64)).reshape(3, 1)], axis=1)
    pts = ((world - Pv[:, 3]) @ Pv[:, :3]).astype(f32)
    rng = np.random.default_rng(59)
    poses = [Pv]
    import map_align_expect as A
    for _ in range(23):
        x = A.about(A.rotation(rng.uniform(-6, 6), rng.normal(size=3)), rng.uniform(-10, 10, 3), world.mean(axis=0))
        poses.append(A.xf_of(x[:, :3] @ Pv[:, :3], x[:, :3] @ Pv[:, 3] + x[:, 3]))
    return pts, np.stack(poses)


@pytest.mark.parametrize("res,color", CASES)
def test_mixed_sources(res, color):
    ctx = Q.mixed_ctx(res, color)
    pts, poses = frame_queries(ctx)
    got = ctx.map_score_poses(pts, poses, R.BAND)                 # (first: the read-outs that build the dictionary settle pending weights)
    d, window = Q.map_dict(ctx, color)
    idx = E.MapIndex(d)
    want = R.np_score(idx, pts, poses, R.BAND)
    s = E.np_sample(idx, R.positions(pts, poses[0]), detail=True)
    is_win = np.array([tuple(k) in window for k in idx.keys.tolist()] + [False])
    from_win, from_store = np.any(is_win[s["slots"]], axis=1) & s["observed"], np.any(~is_win[s["slots"]] & (s["slots"] >= 0), axis=1) & s["observed"]
    print(res, color, "points", len(pts), "observed", int(want["n_obs"][0]), "from the window", int(from_win.sum()), "from the store", int(from_store.sum()), want[:3])
    assert len(pts) >= 1024 and want["n_in"][0] >= len(pts) // 2 and from_win.sum() >= 64 and from_store.sum() >= 64
    assert min(want["n_in"].sum(), want["n_behind"].sum(), want["n_free"].sum(), len(pts) * len(poses) - want["n_obs"].sum()) >= 32
    same_scores(got, want, "mixed")
    if color:                                                     # colour plays no part: the same map without a colour plane gives the same bytes
        plain = Q.mixed_ctx(res, False)
        same_scores(plain.map_score_poses(pts, poses, R.BAND), want, "mixed, no colour plane")
        plain.close()
    ctx.close()


# ---- 3. the edges of the reduction ---------------------------------------------------------------------------------------------------------------------------
def test_reduction_edges():
    pts, poses = many_points(), R.score_poses()
    tsdf, obs = many_samples()
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    for n_points in (1, 63, 64, 65, 255, 256, 257, 4097):
        for n_poses in (1, 3, 300):
            sel = np.arange(n_poses) if n_poses == 300 else np.array([0, 298, 299][:n_poses] if n_poses == 3 else [7])
            want = np.zeros(n_poses, R.SCORE_DTYPE)
            for j, k in enumerate(sel):
                want[j] = R.classify(tsdf[k, :n_points], obs[k, :n_points], R.BAND)
            same_scores(ctx.map_score_poses(pts[:n_points], poses[sel], R.BAND), want, (n_points, n_poses))
            if n_poses == 3:
                assert want["n_obs"][1] == 0 and want["n_obs"][2] == 0      # the NaN pose, the pose beyond the key range
    assert np.isnan(pts[:4097]).any(axis=1).sum() >= 32 and not obs[:, np.isnan(pts[:4097]).any(axis=1)].any()
    ctx.close()


# ---- 4. independence from the expect file --------------------------------------------------------------------------------------------------------------------
def test_scores_from_map_sample():
    """the five integers of a pose, recomputed here from kf_map_sample at the fp64 positions"""
    pts, poses = R.scene()[1], R.score_poses()
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    got = ctx.map_score_poses(pts, poses[:32], R.BAND)
    for k in (0, 3, 5, 17, 31):
        P, p = poses[k], pts.astype(f64)
        w = np.stack([((P[j, 0] * p[:, 0] + P[j, 1] * p[:, 1]) + P[j, 2] * p[:, 2]) + P[j, 3] for j in range(3)], axis=1)
        s = ctx.map_sample(w, want=("tsdf", "weight"))
        seen = s["weight"] > 0
        a = np.abs(s["tsdf"][seen])
        n_in = int(np.count_nonzero(a < f32(R.BAND)))
        n_behind = int(np.count_nonzero((a >= f32(R.BAND)) & (s["tsdf"][seen] < 0)))
        q = int((np.minimum(a, f32(1)) * f32(65536)).astype(np.uint32).astype(np.uint64).sum())
        assert tuple(int(got[k][f]) for f in FIELDS) == (int(seen.sum()), n_in, n_behind, int(seen.sum()) - n_in - n_behind, q), k
    ctx.close()


# ---- 5. the sums ---------------------------------------------------------------------------------------------------------------------------------------------
def sums_cases():
    pose, pts = R.scene()
    poses = np.concatenate([pose[None], R.offset_poses()])
    return pts, poses, np.stack([R.centre_of(pts, P) for P in poses])


def check_sums(got, pts, poses, centres, what):
    for k in range(len(poses)):
        want, mags = R.np_pose_sums(R.cuboid_index(), pts, poses[k], centres[k], R.GATE)
        assert got[k, 28] == want[28] and want[28] >= 256, (what, k, got[k, 28], want[28])
        assert np.all(np.abs(got[k, :28] - want[:28]) <= want[28] * 2.0 ** -52 * mags[:28]), (what, k, np.abs(got[k, :28] - want[:28]), want[28] * 2.0 ** -52 * mags[:28])


def test_pose_sums():
    pts, poses, centres = sums_cases()
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    got = ctx.map_pose_sums(pts, poses, centres, R.GATE)
    check_sums(got, pts, poses, centres, "origin")
    assert np.array_equal(Q.bits(ctx.map_pose_sums(pts, poses, centres, R.GATE)), Q.bits(got))
    # a pose's sums do not depend on the batch
    assert np.array_equal(Q.bits(ctx.map_pose_sums(pts, poses[2:3], centres[2:3], R.GATE)), Q.bits(got[2:3]))
    # 16 500 points: 64 workgroups per pose, lanes with more than one point, points that are not numbers
    big = many_points()
    big_c = np.stack([R.centre_of(pts, P) for P in poses[:2]])
    got_big = ctx.map_pose_sums(big, poses[:2], big_c, 0.75)
    for k in range(2):
        want, mags = R.np_pose_sums(R.cuboid_index(), big, poses[k], big_c[k], 0.75)
        assert got_big[k, 28] == want[28] and want[28] >= 8192
        assert np.all(np.abs(got_big[k, :28] - want[:28]) <= want[28] * 2.0 ** -52 * mags[:28]), k
    other = Q.store_only_ctx(72, False, R.cuboid_map())           # a second context: the same bits
    assert np.array_equal(Q.bits(other.map_pose_sums(pts, poses, centres, R.GATE)), Q.bits(got))
    assert np.array_equal(Q.bits(other.map_pose_sums(big, poses[:2], big_c, 0.75)), Q.bits(got_big))
    other.close()
    ctx.close()
    far = Q.store_only_ctx(64, False, E.shifted(R.cuboid_map(), E.FAR))     # the map at far keys: w - centre is the same number, so are the sums
    got_far = far.map_pose_sums(pts, moved_poses(poses, E.FAR), centres + 8.0 * np.array(E.FAR, f64), R.GATE)
    check_sums(got_far, pts, poses, centres, "far")
    assert np.array_equal(Q.bits(got_far), Q.bits(got))
    far.close()


# ---- 6. the refinement -------------------------------------------------------------------------------------------------------------------------------------------
def refine(ctx, pts, poses, centres, **kw):
    return ctx.map_refine_poses(pts, poses, centres, R.GATE, eps_rot=R.EPS_ROT, eps_trans=R.EPS_TRANS, **kw)


def test_refine_recovers_the_pose():
    """from every start of OFFSETS: CONVERGED, within 4 * 0.1152 = 0.4608 voxels of the true pose at the points (tests/test_map_reloc_cpu.py records the
    0.1152); a batch of 16 gives per pose the bits of 16 single calls"""
    truth, pts = R.scene()
    starts = R.offset_poses()
    centres = np.stack([R.centre_of(pts, P) for P in starts])
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    found, reps = refine(ctx, pts, starts, centres)
    for k in range(len(starts)):
        err = R.pose_error(found[k], truth, pts)
        print("start", k, "off by", R.pose_error(starts[k], truth, pts), "->", err, "iterations", reps[k]["iterations"], "verdict", reps[k]["verdict"])
        assert reps[k]["verdict"] == K.ALIGN_CONVERGED and 1 <= reps[k]["iterations"] <= 25
        assert err <= 4 * R.RECOVERY
    batch = np.concatenate([starts, R.score_poses()[5:17]])
    bc = np.stack([R.centre_of(pts, P) for P in batch])
    all_found, all_reps = refine(ctx, pts, batch, bc)
    assert np.array_equal(Q.bits(all_found[:4]), Q.bits(found))
    verdicts = set()
    for k in range(16):
        one, rep = refine(ctx, pts, batch[k:k + 1], bc[k:k + 1])
        assert np.array_equal(Q.bits(one[0]), Q.bits(all_found[k])), k
        for f in ("iterations", "verdict", "rms"):
            assert rep[0][f] == all_reps[k][f], (k, f)
        assert np.array_equal(Q.bits(rep[0]["sums"]), Q.bits(all_reps[k]["sums"])) and np.array_equal(Q.bits(rep[0]["step"]), Q.bits(all_reps[k]["step"]))
        verdicts.add(rep[0]["verdict"])
    print("verdicts in the batch", verdicts, "iterations", [r["iterations"] for r in all_reps])
    assert len(set(r["iterations"] for r in all_reps)) >= 2       # the poses stopped at different iterations: the running set did shrink
    ctx.close()


# ---- 7. verdicts -----------------------------------------------------------------------------------------------------------------------------------------------
def test_verdicts():
    truth, pts = R.scene()
    starts = R.offset_poses()
    centres = np.stack([R.centre_of(pts, P) for P in starts])
    empty = G.make_ctx(64)
    empty.brick_store_reserve(Q.CAP)
    found, reps = refine(empty, pts, starts, centres)
    assert np.array_equal(Q.bits(found), Q.bits(starts))
    assert all(r["verdict"] == K.ALIGN_FEW_PAIRS and r["iterations"] == 0 and r["sums"][28] == 0 and r["rms"] == 0 for r in reps)
    empty.close()
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    found, reps = refine(ctx, pts, starts, centres, max_iter=0)
    sums = ctx.map_pose_sums(pts, starts, centres, R.GATE)
    assert np.array_equal(Q.bits(found), Q.bits(starts))
    for k, r in enumerate(reps):
        assert r["verdict"] == K.ALIGN_ITER_LIMIT and r["iterations"] == 0 and np.array_equal(Q.bits(r["sums"]), Q.bits(sums[k])) and not r["step"].any()
    found, reps = refine(ctx, pts, starts, centres, min_pairs=len(pts) + 1)      # more pairs asked for than there are points
    assert np.array_equal(Q.bits(found), Q.bits(starts)) and all(r["verdict"] == K.ALIGN_FEW_PAIRS and r["sums"][28] >= 256 for r in reps)
    found, reps = refine(ctx, pts, starts, centres, max_iter=1)
    assert all(r["verdict"] == K.ALIGN_ITER_LIMIT and r["iterations"] == 1 for r in reps) and not np.array_equal(found, starts)
    ctx.close()


# ---- 8. bystanders ---------------------------------------------------------------------------------------------------------------------------------------------
def digest(ctx, color):
    n = C.c_uint32(0)
    st = ctx.lib.kf_triangle_count(ctx.h, C.byref(n))
    return Q.digest(ctx, color) + [repr((st, n.value))]


@pytest.mark.parametrize("res,color", [(64, False), (64, True)])
def test_bystander(res, color):
    """volume planes, sorted store read-out and counts, device pose, model maps and the triangle count are the same bytes before and after the three calls;
    and a context that made them BEFORE anything read the deferred-weight words out goes on exactly as its twin that made none"""
    a, b = Q.mixed_ctx(res, color, defer=1), Q.mixed_ctx(res, color, defer=1)
    pts, poses = frame_queries(b)                                 # placed on the twin: nothing has read A's volume out
    if not color:
        Q.fuse_on(a, (6, 7))
        Q.fuse_on(b, (6, 7))                                      # live words on both
    centres = np.stack([R.positions(pts, P).mean(axis=0) for P in poses[:8]])

    def calls():
        return a.map_score_poses(pts, poses, R.BAND), a.map_pose_sums(pts, poses[:8], centres, R.GATE), refine(a, pts, poses[:8], centres, max_iter=3)
    first = calls()
    assert first[0]["n_in"][0] >= len(pts) // 2 and first[1][0, 28] >= len(pts) // 2
    before = digest(a, color)
    second = calls()
    assert second[0].tobytes() == first[0].tobytes() and np.array_equal(Q.bits(second[1]), Q.bits(first[1])) and np.array_equal(Q.bits(second[2][0]), Q.bits(first[2][0]))
    assert digest(a, color) == before
    assert digest(b, color) == before
    for ctx in (a, b):                                            # the next frame, tracked or not: the same on both
        G.run_frame(ctx, 8, color)
    assert digest(a, color) == digest(b, color)
    a.close()
    b.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib, p = K.load(), K._p
    ctx = Q.store_only_ctx(64, False, R.cuboid_map())
    pts = np.ascontiguousarray(R.scene()[1][:8])
    poses = np.ascontiguousarray(R.offset_poses()[:2]).reshape(2, 12)
    centres = np.full((2, 3), 30.0)
    sc, sums, reps = np.full(2 * 24, 7, np.uint8), np.full(2 * 29, 7.0), np.full(2 * C.sizeof(K.AlignReport), 7, np.uint8)
    kept = poses.copy()
    nan, inf = float("nan"), float("inf")

    def par(gate=1.0, eps_rot=1e-4, eps_trans=1e-3):
        return C.byref(K.RefineParams(5, 1, eps_rot, eps_trans, gate))

    def untouched():
        return (sc == 7).all() and (sums == 7).all() and (reps == 7).all() and np.array_equal(Q.bits(poses), Q.bits(kept))
    for fn in (lib.kf_map_score_poses, lib.kf_map_score_poses_device):
        for a in ((None, 8, p(pts), 2, p(poses), 0.5, p(sc)), (ctx.h, 8, None, 2, p(poses), 0.5, p(sc)), (ctx.h, 8, p(pts), 2, None, 0.5, p(sc)),
                  (ctx.h, 8, p(pts), 2, p(poses), 0.5, None), (ctx.h, 0, p(pts), 2, p(poses), 0.5, p(sc)), (ctx.h, (1 << 24) + 1, p(pts), 2, p(poses), 0.5, p(sc)),
                  (ctx.h, 8, p(pts), 0, p(poses), 0.5, p(sc)), (ctx.h, 8, p(pts), (1 << 20) + 1, p(poses), 0.5, p(sc))):
            assert fn(*a) == ARG, a[1:4:2]
        for band in (nan, inf, 0.0, -0.5, 1.0 + 2.0 ** -20):
            assert fn(ctx.h, 8, p(pts), 2, p(poses), band, p(sc)) == ARG, band
    for a in ((None, 8, p(pts), 2, p(poses), p(centres), 1.0, p(sums)), (ctx.h, 8, None, 2, p(poses), p(centres), 1.0, p(sums)),
              (ctx.h, 8, p(pts), 2, None, p(centres), 1.0, p(sums)), (ctx.h, 8, p(pts), 2, p(poses), None, 1.0, p(sums)),
              (ctx.h, 8, p(pts), 2, p(poses), p(centres), 1.0, None), (ctx.h, 0, p(pts), 2, p(poses), p(centres), 1.0, p(sums)),
              (ctx.h, (1 << 24) + 1, p(pts), 2, p(poses), p(centres), 1.0, p(sums)), (ctx.h, 8, p(pts), 0, p(poses), p(centres), 1.0, p(sums)),
              (ctx.h, 8, p(pts), 4097, p(poses), p(centres), 1.0, p(sums))):
        assert lib.kf_map_pose_sums(*a) == ARG
    for gate in (nan, inf, 0.0, -1.0, 1.0 + 2.0 ** -20):
        assert lib.kf_map_pose_sums(ctx.h, 8, p(pts), 2, p(poses), p(centres), gate, p(sums)) == ARG
        assert lib.kf_map_refine_poses(ctx.h, 8, p(pts), 2, p(poses), p(centres), par(gate=gate), p(reps)) == ARG
    for a in ((None, 8, p(pts), 2, p(poses), p(centres), par(), p(reps)), (ctx.h, 8, None, 2, p(poses), p(centres), par(), p(reps)),
              (ctx.h, 8, p(pts), 2, None, p(centres), par(), p(reps)), (ctx.h, 8, p(pts), 2, p(poses), None, par(), p(reps)),
              (ctx.h, 8, p(pts), 2, p(poses), p(centres), None, p(reps)), (ctx.h, 8, p(pts), 2, p(poses), p(centres), par(), None),
              (ctx.h, 0, p(pts), 2, p(poses), p(centres), par(), p(reps)), (ctx.h, 8, p(pts), 4097, p(poses), p(centres), par(), p(reps)),
              (ctx.h, 8, p(pts), 2, p(poses), p(centres), par(eps_rot=-1e-9), p(reps)), (ctx.h, 8, p(pts), 2, p(poses), p(centres), par(eps_trans=nan), p(reps)),
              (ctx.h, 8, p(pts), 2, p(poses), p(centres), par(eps_rot=inf), p(reps))):
        assert lib.kf_map_refine_poses(*a) == ARG
    for bad_pose, bad_centre in ((nan, 30.0), (inf, 30.0), (None, nan), (None, -inf)):
        q, c = poses.copy(), centres.copy()
        if bad_pose is not None:
            q[1, 5] = bad_pose
        c[1, 2] = bad_centre
        q0 = q.copy()
        assert lib.kf_map_pose_sums(ctx.h, 8, p(pts), 2, p(q), p(c), 1.0, p(sums)) == ARG
        assert lib.kf_map_refine_poses(ctx.h, 8, p(pts), 2, p(q), p(c), par(), p(reps)) == ARG
        assert np.array_equal(Q.bits(q), Q.bits(q0))
    assert untouched()
    # the same arguments, valid: the calls do write
    assert lib.kf_map_score_poses(ctx.h, 8, p(pts), 2, p(poses), 1.0, p(sc)) == 0 and not (sc == 7).all()
    assert lib.kf_map_pose_sums(ctx.h, 8, p(pts), 2, p(poses), p(centres), 1.0, p(sums)) == 0 and not (sums == 7).any()
    assert lib.kf_map_refine_poses(ctx.h, 8, p(pts), 2, p(poses), p(centres), par(), p(reps)) == 0 and not (reps == 7).all()
    ctx.close()
    sc[:], sums[:], reps[:] = 7, 7, 7
    poses[:] = kept
    slab = K.Context(K.camera(*G.CAM), 64, 2.0, G.P["volume_max_weight"], levels=3, slab=(0, 32))
    for fn in (lib.kf_map_score_poses, lib.kf_map_score_poses_device):
        assert fn(slab.h, 8, p(pts), 2, p(poses), 0.5, p(sc)) == STATE
    assert lib.kf_map_pose_sums(slab.h, 8, p(pts), 2, p(poses), p(centres), 1.0, p(sums)) == STATE
    assert lib.kf_map_refine_poses(slab.h, 8, p(pts), 2, p(poses), p(centres), par(), p(reps)) == STATE
    assert untouched()
    slab.close()


# ---- 10. the host class ----------------------------------------------------------------------------------------------------------------------------------------
import test_gpu_map_file as M
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import scene as S

RES, COLOR = 64, False
SIZE = G.SIZES[RES]
TRUNC_M = 5 * SIZE / RES                                          # the apps' truncation: five cells
ROT_STEP = 0.05                                                   # the kidnap lattice's rotation step, radians: about two voxels at the scene's depth


def kidnap_pose(pose, steps):
    """the camera -> window pose `steps` lattice steps (tests/map_reloc_expect.py: KIDNAP_STEPS) off pose: turned about its own centre, moved along the axes"""
    P = R.lattice_pose(np.asarray(pose, f64)[:3], steps, TRUNC_M, ROT_STEP)
    return np.concatenate([P, [[0, 0, 0, 1.0]]])


def fused_app(store=False):
    app = M.make_app(RES, SIZE, G.CAM, COLOR)
    if store:
        app.set_brick_store(Q.CAP)
    for k in range(6):
        assert M.app_frame(app, k, SIZE, G.CAM, COLOR), k
    return app


def kidnap_frames():
    """(the true pose of the kidnapped camera in the first cube's metres, its frame, the true pose and the frame of the camera a moment later)"""
    truth = kidnap_pose(S.trajectory_pose(5, SIZE), R.KIDNAP_STEPS)
    later = kidnap_pose(S.trajectory_pose(5, SIZE), R.KIDNAP_STEPS + np.array([0.05, 0.02, -0.03, 0.02, -0.03, 0.01]))
    mm = [np.ascontiguousarray(S.render_depth_mm(P, G.CAM, SIZE), np.uint16) for P in (truth, later)]
    return truth, mm[0], later, mm[1]


def kidnap_params(**kw):
    return H.reloc_params(trans_step=TRUNC_M, rot_step=ROT_STEP, n=R.KIDNAP_N, top=16, max_points=4096, level=2, min_obs=64, band=R.BAND, gate=R.GATE,
                          accept_inliers=0.5, max_iter=25, min_pairs=64, eps_rot=R.EPS_ROT, eps_trans=R.EPS_TRANS, **kw)


def frame_error_voxels(pose_m, truth_m, mm):
    """how far the frame's level-2 points lie under pose from where they lie under truth, the greatest distance, voxels (R.pose_error in metres / cell)"""
    cols, rows, cx, cy, fx, fy = G.CAM
    z = mm[::4, ::4].astype(f64) / 1000.0
    v, u = np.mgrid[0:rows:4, 0:cols:4]
    p = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=-1)[z > 0]
    a, b = np.asarray(pose_m, f64), np.asarray(truth_m, f64)
    d = (p @ a[:3, :3].T + a[:3, 3]) - (p @ b[:3, :3].T + b[:3, 3])
    return float(np.max(np.linalg.norm(d, axis=1))) / (SIZE / RES)


def test_app_relocalises_a_kidnapped_camera():
    """the camera is 1.3 / -1.3 / 1.2 truncations and 1.3 / -0.8 / -0.3 rotation steps away from the pose the session holds; an explicit lattice covers it.
    relocalise returns true, pose() is within 0.4608 voxels (4 * 0.1152, tests/test_map_reloc_cpu.py) of the scene's ground truth at the frame's points, and
    the following frame is tracked"""
    truth, mm, later, mm_later = kidnap_frames()
    app = fused_app()
    try:
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*G.CAM), RES, SIZE)
        lost_before = ctx.stats()["frames_lost"]
        start = app.pose()[1]
        print("the session's pose is off by", frame_error_voxels(start, truth, mm), "voxels")
        ok, rep = app.relocalise(mm, 6, kidnap_params())
        print({k: rep[k] for k in ("candidates", "points", "best_index", "best_score", "refined_score", "verdict", "iterations", "accepted")})
        assert ok and rep["accepted"] and rep["candidates"] == 3375 and rep["points"] >= 600 and rep["verdict"] == K.ALIGN_CONVERGED
        tracked, pose = app.pose()
        err = frame_error_voxels(pose, truth, mm)
        print("relocalised to", err, "voxels")
        assert tracked and err <= 4 * R.RECOVERY
        assert app.process_frame(mm_later, 7)
        assert ctx.stats()["frames_lost"] == lost_before
        assert frame_error_voxels(app.pose()[1], later, mm_later) <= 1.0     # (tracking goes on from there: within a voxel of the next frame's truth)
    finally:
        app.close()


def test_app_refuses_and_touches_nothing():
    truth, mm, _, _ = kidnap_frames()
    app = fused_app()
    try:
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*G.CAM), RES, SIZE)
        before = M.app_state(app, ctx, COLOR), app.volume_origin(), ctx.stats()["frames_fused"]
        ok, rep = app.relocalise(np.zeros_like(mm), 6, kidnap_params())                     # no measurement in the frame
        assert not ok and rep["points"] == 0 and not rep["accepted"]
        away = np.array(truth, np.float32)
        away[:3, 3] += 50.0                                                                 # a guess from which no candidate sees any of the map
        ok, rep = app.relocalise(mm, 6, kidnap_params(guess=away))
        assert not ok and rep["points"] >= 600 and rep["candidates"] == 3375 and not rep["accepted"]
        after = M.app_state(app, ctx, COLOR), app.volume_origin(), ctx.stats()["frames_fused"]
        assert before[0][0] == after[0][0] and np.array_equal(before[0][1], after[0][1]) and before[1:] == after[1:]
        assert all(np.array_equal(x, y) for x, y in zip(before[0][2], after[0][2]))
        assert M.app_frame(app, 6, SIZE, G.CAM, COLOR)                                      # the session goes on as if nothing had been asked
    finally:
        app.close()


def test_app_places_the_window_where_the_pose_looks():
    """with a store reserved and the window shifted away, the found pose looks into another frame than the window's: the window is captured and placed there,
    and pose() + origin still matches the ground truth"""
    truth, mm, later, mm_later = kidnap_frames()
    app = fused_app(store=True)
    try:
        assert app.shift_volume(*Q.SHIFT) and app.volume_origin() == Q.SHIFT
        ok, rep = app.relocalise(mm, 6, kidnap_params())
        assert ok and rep["accepted"]
        origin = app.volume_origin()
        assert origin != Q.SHIFT and all(o % 8 == 0 for o in origin)
        tracked, pose = app.pose()
        world = np.array(pose, f64)
        world[:3, 3] += np.array(origin, f64) * (SIZE / RES)
        err = frame_error_voxels(world, truth, mm)
        print("window placed at", origin, "relocalised to", err, "voxels")
        assert tracked and err <= 4 * R.RECOVERY
        assert app.process_frame(mm_later, 7)
    finally:
        app.close()


def test_slab_application_refuses():
    sl = H.SlabsApp(64, 2.0, G.CAM, [0, 32, 64])
    try:
        with pytest.raises(K.KfError):
            sl.relocalise(np.zeros((G.CAM[1], G.CAM[0]), np.uint16), 0)
    finally:
        sl.close()
