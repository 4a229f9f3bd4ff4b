"""CPU-only: the yardstick of relocalisation (tests/map_reloc_expect.py) held against what is known in closed form on its analytic cuboid, and the point and
pose sets the GPU test uses shown to hold enough of every class.  Nothing here calls the library.

Recorded here for tests/test_gpu_map_reloc.py: np_refine from every start of OFFSETS (0.77 to 3.26 voxels off at the points) ends CONVERGED within
0.1152 voxels of the true pose at the points -- the error of the trilinear field near the cuboid's edges, not of the loop: the true pose itself refines to
0.115.  The GPU test's bound is four times that, 0.4608 voxels: the margin covers the different fold order and one more or one fewer iteration."""
import numpy as np

import map_query_expect as E
import map_reloc_expect as R

f32 = np.float32
RECOVERY = R.RECOVERY                                             # the measured recovery error, voxels (the docstring)


def face_points(margin):
    """the points that lie on the cuboid's largest visible face at least `margin` voxels from its edges: (the points, the face's outward normal in the world)"""
    pose, pts = R.scene()
    local = (R.positions(pts, pose) - R.CUBOID_CENTRE) @ R.CUBOID_R
    q = np.abs(local) - R.CUBOID_HALF
    axis = 2                                                      # the faces z = +-7 are the largest; the camera sees z = -7
    on = (np.abs(q[:, axis]) < 0.05) & np.all(np.delete(q, axis, axis=1) < -margin, axis=1)
    sign = np.sign(local[on, axis])
    assert len(sign) >= 32 and np.all(sign == sign[0]), len(sign)
    return pts[on], sign[0] * R.CUBOID_R[:, axis]


def test_true_pose_and_a_push_along_a_face_normal():
    pose, pts = R.scene()
    s = R.np_score(R.cuboid_index(), pts, pose, R.BAND)[0]
    assert s["n_obs"] == len(pts) == s["n_in"] and s["n_behind"] == 0 and s["n_free"] == 0 and len(pts) >= 257
    # a point lies within sqrt(3) 2^-9 voxels of its hit (the 2^-8 lattice), a hit on a plane is exact to rounding, the field of a face away from the edges
    # is linear and the trilinear sample exact on it: |tsdf| <= 0.0034 / 4 + rounding, and one unit of q for the truncation
    tol = 2e-3
    face, normal = face_points(6.0)
    base = R.np_score(R.cuboid_index(), face, pose, R.BAND)[0]
    assert base["sum_q"] / base["n_obs"] / 65536 < tol
    for d in (0.5, 1.5, 3.0, -1.5):
        pushed = R.moved_pose(pose, (0, 0, 0))
        pushed[:, 3] += d * normal
        got = R.np_score(R.cuboid_index(), face, pushed, R.BAND)[0]
        assert got["n_obs"] == len(face)
        assert abs(got["sum_q"] / got["n_obs"] / 65536 - abs(d) / E.TRUNC) < tol, d
        inb = abs(d) / E.TRUNC < R.BAND
        assert got["n_in"] == (len(face) if inb else 0) and got["n_behind"] == (len(face) if not inb and d < 0 else 0) and got["n_free"] == (len(face) if not inb and d > 0 else 0)


def test_row_predicts_the_change_under_a_small_twist():
    """e' = e - J . xi under pose <- T(c) exp(xi) T(-c) pose, against a finite difference, on a face's interior where the field is linear: what is left is the
    second order of the rotation, |omega|^2 |x| |g| <= 1e-6 * 40 * 0.25, and the rounding of two fp32 values"""
    import map_align_expect as A
    pose, _ = R.scene()
    face, _ = face_points(6.0)
    centre = R.centre_of(face, pose)
    J, e, part = R.np_pose_terms(R.cuboid_index(), face, pose, centre, R.GATE)
    assert part.all()
    rng = np.random.default_rng(3)
    for _ in range(4):
        xi = np.concatenate([rng.uniform(-1, 1, 3) * 5e-4, rng.uniform(-1, 1, 3) * 2e-2])
        Ex, u = A.np_exp(xi)
        moved = A.xf_of(Ex @ pose[:, :3], Ex @ (pose[:, 3] - centre) + centre + u)
        _, e2, part2 = R.np_pose_terms(R.cuboid_index(), face, moved, centre, R.GATE)
        assert part2.all()
        pred = e.astype(np.float64) - J.astype(np.float64) @ xi
        assert np.max(np.abs(e2 - pred)) < 2e-5
        assert np.max(np.abs(e2 - e)) > 2e-4                       # (the twist did move the values: ten times the tolerance)


def test_refinement_recovers_every_start_and_the_sets_hold_every_class():
    pose, pts = R.scene()
    out, err = R.refine_expected()
    start = [R.pose_error(P, pose, pts) for P in R.offset_poses()]
    print("starts off by", start, "recovered to", err, "verdicts", [(o[1], o[2]) for o in out])
    assert min(start) > 0.5 and max(start) > 3.0
    assert all(o[1] == R.CONVERGED for o in out)
    assert err <= RECOVERY
    sc = R.np_score(R.cuboid_index(), pts, R.score_poses(), R.BAND)
    total = {k: int(sc[k].sum()) for k in ("n_obs", "n_in", "n_behind", "n_free")}
    unobserved = len(pts) * len(sc) - total["n_obs"]
    print(total, "unobserved", unobserved)
    assert min(total["n_in"], total["n_behind"], total["n_free"], unobserved) >= 32
    assert np.all(sc["n_obs"] == sc["n_in"] + sc["n_behind"] + sc["n_free"]) and np.all(sc["n_obs"][-2:] == 0)
    assert np.argmax(2 * sc["n_in"].astype(np.int64) - sc["n_obs"]) in (0, 1)   # the true pose, or the start half a voxel off it, ranks first


def test_positions_are_exact_at_the_far_keys():
    pose, pts = R.scene()
    for P in R.score_poses()[:-2]:
        assert np.array_equal(R.positions(pts, R.moved_pose(P, E.FAR)) - 8.0 * np.array(E.FAR, np.float64), R.positions(pts, P))


def test_the_kidnap_lies_within_half_a_step_of_a_node_and_refines_from_it():
    """the offsets tests/test_gpu_map_reloc.py kidnaps the camera by (KIDNAP_STEPS, in lattice steps) lie within half a step of KIDNAP_NODE on every axis, inside
    the lattice KIDNAP_N; on the analytic cuboid np_refine from that node comes back to the true pose within the recorded recovery error, and so does the
    whole search -- lattice, scores, rank, the best 16 refined, scored again, the best of them"""
    assert np.all(np.abs(R.KIDNAP_STEPS - R.KIDNAP_NODE) <= 0.5) and np.all(np.abs(R.KIDNAP_NODE) <= np.array(R.KIDNAP_N))
    assert np.linalg.norm(R.KIDNAP_STEPS[:3]) >= 2.0              # several truncations of translation (a step is one truncation)
    truth, pts = R.scene()
    start, trans, rot = R.kidnap_case()
    assert R.pose_error(start, truth, pts) > 8.0
    node = R.lattice_pose(start, R.KIDNAP_NODE, trans, rot)
    assert np.allclose(R.lattice_pose(start, R.KIDNAP_STEPS, trans, rot), truth, rtol=0, atol=1e-12)
    found, verdict, _, _, _ = R.np_refine(R.cuboid_index(), pts, node, R.centre_of(pts, node), R.GATE, eps_rot=R.EPS_ROT, eps_trans=R.EPS_TRANS)
    print("node off by", R.pose_error(node, truth, pts), "->", R.pose_error(found, truth, pts))
    assert verdict == R.CONVERGED and R.pose_error(found, truth, pts) <= R.RECOVERY
    lattice = R.np_lattice(start, R.KIDNAP_N, trans, rot)
    assert len(lattice) == 3375 and np.array_equal(lattice[len(lattice) // 2], start)
    scores = R.np_score(R.cuboid_index(), pts, lattice, R.BAND)
    best, eligible = R.np_rank(scores, 64, 16)
    assert eligible >= 16
    mean = pts.astype(np.float64).mean(axis=0)
    refined = np.stack([R.np_refine(R.cuboid_index(), pts, lattice[k], lattice[k][:, :3] @ mean + lattice[k][:, 3], R.GATE, min_pairs=64, eps_rot=R.EPS_ROT,
                                    eps_trans=R.EPS_TRANS)[0] for k in best])
    again = R.np_score(R.cuboid_index(), pts, refined, R.BAND)
    win = R.np_rank(again, 64, 1)[0][0]
    print("the search's winner", again[win], R.pose_error(refined[win], truth, pts))
    assert again[win]["n_in"] == len(pts) and R.pose_error(refined[win], truth, pts) <= R.RECOVERY
