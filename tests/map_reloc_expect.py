"""The yardstick of relocalisation (kf_map_score_poses, kf_map_pose_sums, kf_map_refine_poses), not collected: include/hybkf.h's rule restated in numpy over
map_query_expect.np_sample, one analytic map and the point and pose sets the CPU and the GPU test share.  Nothing here calls the library.

float64 for a point's position under a pose (one rounded operation per operation written), np_sample for the value and the gradient, float32 arrays for x
and the row (asserted by dtype), the products formed in float64 -- exact, both factors being float32 -- and added with math.fsum, so every sum is the
correctly rounded sum of its terms.

The map is a cuboid with three different half extents, turned off the axes, so that a pose is determined by the points on three of its faces.  Every point
coordinate and every translation is a multiple of 2^-8, every rotation entry a multiple of 2^-16 (such a matrix is orthonormal to about 1e-5 only: poses are
not checked for being rigid), so that a position w is exact at the origin AND at map_query_expect.FAR: a map moved by whole bricks gives the same bytes."""
import functools
import math

import numpy as np

import map_align_expect as A
import map_query_expect as E

f32, f64 = np.float32, np.float64
SCORE_DTYPE = np.dtype([("n_obs", "<u4"), ("n_in", "<u4"), ("n_behind", "<u4"), ("n_free", "<u4"), ("sum_q", "<u8")])
CONVERGED, ITER_LIMIT, FEW_PAIRS, SINGULAR = A.CONVERGED, A.ITER_LIMIT, A.FEW_PAIRS, A.SINGULAR
BAND = 0.5                                                        # the scores' band, tsdf units: two voxels of the maps' truncation of four
GATE = 1.0                                                        # the sums' gate
# the refinement's stopping rule in the tests.  The trilinear field's gradient jumps at every cell border, so on this map the Gauss-Newton steps do not fall to
# rounding level: they end in a cycle of about 5e-5 rad and 3e-4 voxels (measured with np_refine, eps 1e-9, 25 iterations, every start of OFFSETS), three
# orders below the error of the result itself.  The eps stand four to five times above that cycle.
EPS_ROT, EPS_TRANS = 2.5e-4, 1e-3
# np_refine's recovery error from every start of OFFSETS, voxels at the points, as measured and asserted by tests/test_map_reloc_cpu.py; the GPU test's bound
# is four times this
RECOVERY = 0.1152

CUBOID_HALF, CUBOID_CENTRE = np.array([14.0, 10.0, 7.0]), np.array([32.3, 31.1, 30.7])
CUBOID_R = A.rotation(20.0, (1, 2, 3))                            # the cuboid's axes in the world


def cuboid_sdf(p):
    q = np.abs((p - CUBOID_CENTRE) @ CUBOID_R) - CUBOID_HALF
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


@functools.lru_cache(maxsize=None)
def cuboid_map():
    """(shared: nobody writes into it)"""
    return E._analytic(cuboid_sdf, 0, 8)


@functools.lru_cache(maxsize=None)
def cuboid_index():
    return E.MapIndex(cuboid_map())


def quantised_pose(r, t):
    return A.xf_of(E._q(r, 16), E._q(t, 8))


@functools.lru_cache(maxsize=None)
def scene():
    """(the true pose [R | t] (3, 4), camera -> world voxels; the points (n, 3) float32 in the camera frame): the hits of a 40 x 30 camera that looks at a
    corner of the cuboid and sees three of its faces, brought into the camera frame"""
    eye = CUBOID_CENTRE + CUBOID_R @ np.array([30.0, 26.0, -24.0])
    z = E._unit(CUBOID_CENTRE - eye)
    x = E._unit(np.cross(np.array([0.0, 1.0, 0.0]), z))
    pose = quantised_pose(np.stack([x, np.cross(z, x), z], axis=1), eye)
    v, u = np.mgrid[0:30, 0:40]
    local = np.stack([(u.reshape(-1) - 19.5) / 36.0, (v.reshape(-1) - 14.5) / 36.0, np.ones(1200)], axis=1)
    o = np.broadcast_to(pose[:, 3], (1200, 3)).copy()
    o, d, t0, t1 = E._rays(o, o + 10.0 * (local @ pose[:, :3].T), 8.0, 90.0)
    r = E.np_cast(cuboid_index(), o, d, t0, t1, E.STEP)
    hit = r["status"] == E.HIT
    world = o[hit] + (r["t"][hit][:, None] * d[hit]).astype(f64)
    pts = E._q((world - pose[:, 3]) @ np.linalg.inv(pose[:, :3]).T, 8).astype(f32)
    pts.setflags(write=False)
    pose.setflags(write=False)
    return pose, pts


def offset_pose(pose, deg, axis, t):
    """the pose turned by deg about axis through the cuboid's centre and moved by t voxels, quantised"""
    x = A.about(A.rotation(deg, axis), t, CUBOID_CENTRE)
    return quantised_pose(x[:, :3] @ pose[:, :3], x[:, :3] @ pose[:, 3] + x[:, 3])


# the starts kf_map_refine_poses is tested from: (degrees, axis, translation in voxels) off the true pose
OFFSETS = [(1.0, (1, 0, 0), (0.5, -0.25, 0.25)), (2.0, (0, 1, 0), (-1.0, 0.5, 0.75)), (3.0, (1, 2, 3), (1.5, -1.0, 0.5)), (4.0, (-2, 1, 1), (-1.5, 1.25, -1.0))]


def offset_poses():
    pose, _ = scene()
    return np.stack([offset_pose(pose, *o) for o in OFFSETS])


@functools.lru_cache(maxsize=None)
def score_poses():
    """300 poses: the true one, the refine starts, then poses pushed up to 8 voxels along and across the view and turned up to 12 degrees -- points end up in
    the band, behind the surface, in free space and where nobody observed -- and, last, one with a NaN and one 2^24 voxels away"""
    pose, _ = scene()
    rng = np.random.default_rng(53)
    out = [pose] + list(offset_poses())
    while len(out) < 298:
        out.append(offset_pose(pose, rng.uniform(-12, 12), rng.normal(size=3), rng.uniform(-8, 8, 3)))
    nan, far = pose.copy(), pose.copy()
    nan[1, 1] = np.nan
    far[0, 3] = 2.0 ** 24
    a = np.stack(out + [nan, far])
    a.setflags(write=False)
    return a


def positions(points, pose):
    """w_j = ((R[j][0] x + R[j][1] y) + R[j][2] z) + t[j], float64"""
    p = np.asarray(points, f32).reshape(-1, 3).astype(f64)
    P = np.asarray(pose, f64).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((P[j, 0] * p[:, 0] + P[j, 1] * p[:, 1]) + P[j, 2] * p[:, 2]) + P[j, 3] for j in range(3)], axis=1)


def classify(tsdf, observed, band):
    """the five integers of one pose from the sample's tsdf and observed flag"""
    band = f32(band)
    a = np.abs(tsdf)
    assert a.dtype == f32
    inb = observed & (a < band)
    behind = observed & ~inb & (tsdf < 0)
    q = (np.minimum(a, f32(1)) * f32(65536)).astype(np.uint32)   # (exact product, truncated)
    n_obs, n_in, n_behind = int(np.count_nonzero(observed)), int(np.count_nonzero(inb)), int(np.count_nonzero(behind))
    return n_obs, n_in, n_behind, n_obs - n_in - n_behind, int(q[observed].astype(np.uint64).sum())


def np_score(m, points, poses, band):
    m = E._index(m)
    poses = np.asarray(poses, f64).reshape(-1, 3, 4)
    out = np.zeros(len(poses), SCORE_DTYPE)
    for k, P in enumerate(poses):
        s = E.np_sample(m, positions(points, P))
        out[k] = classify(s["tsdf"], s["observed"], band)
    return out


def np_pose_terms(m, points, pose, centre, gate):
    """the rows of the points that take part: (J (n, 6) float32, e (n,) float32, which points)"""
    w = positions(points, pose)
    s = E.np_sample(E._index(m), w)
    part = s["observed"] & (np.abs(s["tsdf"]) < f32(gate))
    x = (w[part] - np.asarray(centre, f64)).astype(f32)
    g = s["grad"][part]
    J = np.stack([x[:, 1] * g[:, 2] - x[:, 2] * g[:, 1], x[:, 2] * g[:, 0] - x[:, 0] * g[:, 2], x[:, 0] * g[:, 1] - x[:, 1] * g[:, 0], g[:, 0], g[:, 1], g[:, 2]], axis=1)
    e = -s["tsdf"][part]
    assert J.dtype == f32 and e.dtype == f32
    return J, e, part


def np_pose_sums(m, points, pose, centre, gate):
    """map_align_expect.np_row_sums of np_pose_terms"""
    return A.np_row_sums(*np_pose_terms(m, points, pose, centre, gate)[:2])


def np_refine(m, points, pose, centre, gate, max_iter=25, min_pairs=100, eps_rot=1e-9, eps_trans=1e-9):
    """kf_map_refine_poses' loop for one pose over np_pose_sums: (pose, verdict, iterations, the last evaluation's sums, the last step)"""
    m = E._index(m)
    return A.np_gauss_newton(lambda x: np_pose_sums(m, points, x, centre, gate)[0], pose, centre, max_iter, min_pairs, eps_rot, eps_trans)


def centre_of(points, pose):
    """the mean of the points under the pose, on the 2^-8 lattice"""
    return E._q(positions(points, pose).mean(axis=0), 8)


def pose_error(pose, truth, points):
    """how far the points lie under `pose` from where they lie under `truth`, the greatest distance, voxels"""
    return float(np.max(np.linalg.norm(positions(points, pose) - positions(points, truth), axis=1)))


@functools.lru_cache(maxsize=None)
def refine_expected():
    """np_refine from every start of OFFSETS: a list of (pose, verdict, iterations), and the greatest pose_error against the true pose"""
    truth, pts = scene()
    out = [np_refine(cuboid_index(), pts, P, centre_of(pts, P), GATE, eps_rot=EPS_ROT, eps_trans=EPS_TRANS)[:3] for P in offset_poses()]
    return out, max(pose_error(r[0], truth, pts) for r in out)


def moved_pose(pose, db):
    """the pose of the same camera in a map moved by db bricks: exact, t is on the 2^-8 lattice"""
    P = np.array(pose, f64).reshape(3, 4)
    P[:, 3] += 8.0 * np.asarray(db, f64)
    return P


# ---- the host functions restated (host/reloc_search.hpp) ---------------------------------------------------------------------------------------------------
def np_points(verts, cell, max_points):
    """hkf_reloc_points: valid vertices (z != 0) in row-major order, subsampled at floor(i * count / max_points), float32 of the float64 quotient; the median:
    element count // 2 of the sorted valid z"""
    v = np.asarray(verts, f32).reshape(-1, 4)
    valid = np.flatnonzero(v[:, 2] != 0)
    count = len(valid)
    if count == 0 or max_points == 0:
        return np.zeros((0, 3), f32), 0.0
    med = float(np.sort(v[valid, 2])[count // 2])
    if count > max_points:
        valid = valid[(np.arange(max_points, dtype=np.int64) * count) // max_points]
    return (v[valid, :3].astype(f64) / f64(f32(cell))).astype(f32), med


def np_lattice(centre, n, trans_step, rot_step):
    """hkf_reloc_lattice: R = Rc exp(omega^), t = tc + index * trans_step; translation outermost, ia slowest, jc fastest"""
    c = np.asarray(centre, f64).reshape(3, 4)
    out = []
    ax = [range(-k, k + 1) for k in n]
    for ia in ax[0]:
        for ib in ax[1]:
            for ic in ax[2]:
                for ja in ax[3]:
                    for jb in ax[4]:
                        for jc in ax[5]:
                            Ex, _ = A.np_exp(np.array([ja * rot_step, jb * rot_step, jc * rot_step, 0.0, 0.0, 0.0]))
                            out.append(A.xf_of(c[:, :3] @ Ex, c[:, 3] + np.array([ia, ib, ic], f64) * trans_step))
    return np.stack(out)


def np_rank(scores, min_obs, m):
    """hkf_reloc_rank: (the best indices, the number eligible): key 2 n_in - n_obs larger first, then the smaller sum_q, then the smaller index"""
    sc = np.asarray(scores)
    idx = np.flatnonzero(sc["n_obs"] >= min_obs)
    key = 2 * sc["n_in"][idx].astype(np.int64) - sc["n_obs"][idx].astype(np.int64)
    order = np.lexsort((idx, sc["sum_q"][idx], -key))
    return idx[order][:m].astype(np.uint32), len(idx)


# ---- the kidnap: where the camera really is, in lattice steps off the pose the search starts from ----------------------------------------------------------
KIDNAP_STEPS = np.array([1.3, -1.3, 1.2, 1.3, -0.8, -0.3])        # three translation axes, three rotation axes: within half a step of node (1, -1, 1, 1, -1, 0)
KIDNAP_NODE = np.array([1, -1, 1, 1, -1, 0])
KIDNAP_N = (2, 2, 2, 1, 1, 1)                                     # the lattice that covers it: 125 * 27 = 3 375 candidates


def lattice_pose(centre, steps, trans_step, rot_step):
    """the pose `steps` (6, fractions allowed) lattice steps off centre, by the lattice's rule"""
    c = np.asarray(centre, f64).reshape(3, 4)
    Ex, _ = A.np_exp(np.concatenate([np.asarray(steps[3:], f64) * rot_step, np.zeros(3)]))
    return A.xf_of(c[:, :3] @ Ex, c[:, 3] + np.asarray(steps[:3], f64) * trans_step)


@functools.lru_cache(maxsize=None)
def kidnap_case():
    """on the analytic cuboid: (the pose the search starts from, translation step, rotation step) such that the scene's true pose lies KIDNAP_STEPS off it:
    steps of one truncation and atan(truncation / median depth)"""
    truth, pts = scene()
    trans, rot = E.TRUNC, math.atan(E.TRUNC / float(np.sort(pts[:, 2])[len(pts) // 2]))
    # truth = start . lattice offset: R_t = R_s exp(w^), t_t = t_s + d  =>  R_s = R_t exp(-w^), t_s = t_t - d
    Ex, _ = A.np_exp(np.concatenate([-KIDNAP_STEPS[3:] * rot, np.zeros(3)]))
    start = A.xf_of(truth[:, :3] @ Ex, truth[:, 3] - KIDNAP_STEPS[:3] * trans)
    return start, trans, rot
