"""The yardstick of map alignment: the rule of kf_align_brick_store (include/hybkf.h) restated in numpy, the analytic maps the tests align, and the
Gauss-Newton loop over the restatement's own sums.  Nothing here calls the library.

float64 for a brick's base corner and for the bracket of x; float32 arrays with one rounded operation per operation for the position, the value, the
gradient and the row (asserted by dtype); the products formed in float64 -- exact, both factors being float32 -- and added with math.fsum, so every sum is
the correctly rounded sum of its terms.  A map is (keys (n, 3) int32, tsdf (n, 8, 8, 8) float32 in (z, y, x) order, weight likewise, colour or None), as
everywhere in the tests."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
CONVERGED, ITER_LIMIT, FEW_PAIRS, SINGULAR = 0, 1, 2, 3
EPS_ROT_MIN, EPS_TRANS_MIN = 2.0 ** -23, 2.0 ** -18               # what the fp32 rule resolves: a smaller eps is raised to these (include/hybkf.h)
TRI = [(a, b) for a in range(6) for b in range(a, 6)]             # the order of the 21 products


def rotation(deg, axis):
    """Rodrigues, float64"""
    k = np.asarray(axis, f64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(a) * np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * np.outer(k, k)


def xf_of(r, t):
    return np.concatenate([np.asarray(r, f64), np.asarray(t, f64).reshape(3, 1)], axis=1)


def inverse(xf):
    r, t = xf[:, :3], xf[:, 3]
    return xf_of(r.T, -r.T @ t)


def compose(a, b):
    """a after b"""
    return xf_of(a[:, :3] @ b[:, :3], a[:, :3] @ b[:, 3] + a[:, 3])


def about(r, t, c):
    """x -> c + R (x - c) + t"""
    c = np.asarray(c, f64)
    return xf_of(r, c - r @ c + np.asarray(t, f64))


def moved_by_bricks(xf, shift):
    """the transform between the same two maps after both were moved by `shift` bricks: T(s) xf T(-s), s = 8 shift"""
    s = 8.0 * np.asarray(shift, f64)
    return xf_of(xf[:, :3], xf[:, 3] + s - xf[:, :3] @ s)


def halfway(xf):
    """the transform half of the way from the identity to xf: half the rotation angle about the same axis, half the translation"""
    r = xf[:, :3]
    w = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    s, c = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(r) - 1.0)
    ang = np.arctan2(s, c)
    return xf_of(rotation(np.rad2deg(ang) / 2, w) if s > 0 else np.eye(3), xf[:, 3] / 2)


# ---- the analytic maps ---------------------------------------------------------------------------------------------------------------------------------
BOX_HALF, BOX_CENTRE, BAND, RES = np.array([14.0, 10.0, 7.0]), np.array([32.3, 31.1, 30.7]), 4.0, 64
MOVES = {                                                          # X: degrees about (1, 2, 3), translation in voxels
    "2deg": (2.0, (0.8, -0.5, 0.3)),
    "5deg": (5.0, (2.0, -1.5, 1.0)),
    "10deg": (10.0, (3.0, -2.5, 2.0)),
}


def move(name):
    deg, t = MOVES[name]
    return about(rotation(deg, (1, 2, 3)), t, BOX_CENTRE)


def box_sdf(p):
    q = np.abs(p - BOX_CENTRE) - BOX_HALF
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


def slab_sdf(p):
    """two parallel planes: the slab |z - centre| <= half extent"""
    return np.abs(p[..., 2] - BOX_CENTRE[2]) - BOX_HALF[2]


def analytic_planes(x=None, sdf=box_sdf):
    """the scene moved by x (3x4, None: not moved), sampled at the voxel centres of [0, 64)^3: dense (tsdf, weight) in (z, y, x) order.
    tsdf = min(1, sdf / 4) as float32, weight 1 where sdf > -4, elsewhere unobserved: zeros"""
    z, y, xx = np.meshgrid(*(np.arange(RES) + 0.5,) * 3, indexing="ij")
    p = np.stack([xx, y, z], -1)
    if x is not None:
        inv = inverse(x)
        p = p @ inv[:, :3].T + inv[:, 3]
    d = sdf(p)
    seen = d > -BAND
    return np.where(seen, np.minimum(1.0, d / BAND), 0.0).astype(f32), seen.astype(f32)


def bricked(t, w, shift=(0, 0, 0)):
    """dense planes standing at the origin -> the map of the bricks with a weight > 0, sorted (z, y, x), its keys moved by `shift` bricks (what
    test_gpu_map_resample.rebrick gives at the origin; restated so that the CPU tests import no GPU test module)"""
    keys, bt, bw = [], [], []
    for z in range(0, t.shape[0], 8):
        for y in range(0, t.shape[1], 8):
            for x in range(0, t.shape[2], 8):
                if np.any(w[z:z + 8, y:y + 8, x:x + 8] > 0):
                    keys.append((x // 8 + shift[0], y // 8 + shift[1], z // 8 + shift[2]))
                    bt.append(t[z:z + 8, y:y + 8, x:x + 8]); bw.append(w[z:z + 8, y:y + 8, x:x + 8])
    return np.array(keys, np.int32).reshape(-1, 3), np.ascontiguousarray(np.stack(bt)), np.ascontiguousarray(np.stack(bw)), None


_ANALYTIC = {}


def analytic_map(name=None, shift=(0, 0, 0), sdf=box_sdf):
    """map A (name None: the scene itself) or map B (the scene moved by MOVES[name]); computed once and shared, nobody writes into the arrays"""
    key = (name, tuple(shift), sdf.__name__)
    if key not in _ANALYTIC:
        m = bricked(*analytic_planes(move(name) if name else None, sdf), shift=shift)
        for a in m[:3]:
            a.setflags(write=False)
        _ANALYTIC[key] = m
    return _ANALYTIC[key]


def slab_maps():
    """two parallel planes only: (the slab, the same slab moved by (0.4, -0.3, 0.6) voxels without a turn)"""
    if "slab" not in _ANALYTIC:
        _ANALYTIC["slab"] = (bricked(*analytic_planes(None, slab_sdf)), bricked(*analytic_planes(xf_of(np.eye(3), (0.4, -0.3, 0.6)), slab_sdf)))
    return _ANALYTIC["slab"]


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------------------
def dense_of(m, pad=1):
    """map m as dense (tsdf, weight) over its keys' box, `pad` bricks wider on every side: (origin in voxels (x, y, z), tsdf, weight)"""
    lo, hi = m[0].min(axis=0).astype(np.int64) - pad, m[0].max(axis=0).astype(np.int64) + 1 + pad
    n = (hi - lo)[::-1] * 8
    t, w = np.zeros(n, f32), np.zeros(n, f32)
    for i, k in enumerate(m[0].tolist()):
        x, y, z = ((k[j] - lo[j]) * 8 for j in range(3))
        t[z:z + 8, y:y + 8, x:x + 8], w[z:z + 8, y:y + 8, x:x + 8] = m[1][i], m[2][i]
    return lo * 8, t, w


def np_rows(dst, src, xf, centre):
    """every voxel of the held map `dst` that takes part at xf: (J (n, 6) float32, e (n,) float32)"""
    xf, centre = np.asarray(xf, f64), np.asarray(centre, f64)
    r, t = xf[:, :3], xf[:, 3]
    keys = dst[0].astype(np.int64)
    so, st, sw = dense_of(src, pad=1)
    # per brick, float64:  a = 8 K + 0.5 - t;  c_j = ((R[0][j] a_0 + R[1][j] a_1) + R[2][j] a_2) - 0.5
    a = 8.0 * keys.astype(f64) + 0.5 - t
    ib, fb = np.empty((len(keys), 3), np.int64), np.empty((len(keys), 3), f32)
    fit = np.ones(len(keys), bool)
    for j in range(3):
        c = ((r[0, j] * a[:, 0] + r[1, j] * a[:, 1]) + r[2, j] * a[:, 2]) - 0.5
        fl = np.floor(c)
        fit &= (fl >= -1073741824.0) & (fl < 1073741824.0)
        frac = (c - fl).astype(f32)
        up = frac == f32(1)
        ib[:, j], fb[:, j] = np.where(fit, fl, 0).astype(np.int64) + up, np.where(up, f32(0), frac)
    rf = r.astype(f32)
    lz, ly, lx = (v.astype(f32)[None] for v in np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"))
    l = (lx, ly, lz)
    i, f, x = [], [], []
    for j in range(3):
        u = ((rf[0, j] * lx + rf[1, j] * ly) + rf[2, j] * lz) + fb[:, j, None, None, None]
        assert u.dtype == f32
        n = np.floor(u)
        f.append(u - n)
        i.append(ib[:, j, None, None, None] + n.astype(np.int64))
        xb = (8.0 * keys[:, j].astype(f64) + 0.5 - centre[j]).astype(f32)
        x.append(xb[:, None, None, None] + l[j])
    assert f[0].dtype == f32 and x[0].dtype == f32
    # the held side, then the eight corners
    td = dst[1].astype(f32)
    part = (dst[2] > 0) & (np.abs(td) < f32(1)) & fit[:, None, None, None]
    shape = np.array(st.shape)
    v = []
    for k in range(8):
        cx, cy, cz = i[0] + (k & 1) - so[0], i[1] + ((k >> 1) & 1) - so[1], i[2] + (k >> 2) - so[2]
        inside = (cx >= 0) & (cx < shape[2]) & (cy >= 0) & (cy < shape[1]) & (cz >= 0) & (cz < shape[0])
        cx, cy, cz = np.clip(cx, 0, shape[2] - 1), np.clip(cy, 0, shape[1] - 1), np.clip(cz, 0, shape[0] - 1)
        ct = st[cz, cy, cx]
        part &= inside & (sw[cz, cy, cx] > 0) & (np.abs(ct) < f32(1))
        v.append(ct)
    lerp = lambda p, q, w: p + w * (q - p)
    a4 = [lerp(v[2 * k], v[2 * k + 1], f[0]) for k in range(4)]
    b2 = [lerp(a4[0], a4[1], f[1]), lerp(a4[2], a4[3], f[1])]
    phi = lerp(b2[0], b2[1], f[2])
    d4 = [v[2 * k + 1] - v[2 * k] for k in range(4)]
    gx = lerp(lerp(d4[0], d4[1], f[1]), lerp(d4[2], d4[3], f[1]), f[2])
    gy = lerp(a4[1] - a4[0], a4[3] - a4[2], f[2])
    gz = b2[1] - b2[0]
    gd = [(rf[k, 0] * gx + rf[k, 1] * gy) + rf[k, 2] * gz for k in range(3)]
    J = [x[1] * gd[2] - x[2] * gd[1], x[2] * gd[0] - x[0] * gd[2], x[0] * gd[1] - x[1] * gd[0], gd[0], gd[1], gd[2]]
    e = phi - td
    assert all(q.dtype == f32 for q in J) and e.dtype == f32 and phi.dtype == f32
    return np.stack([q[part] for q in J], -1), e[part]


def np_row_sums(J, e):
    """(the 29 sums of the rows (J, e), float64: each the correctly rounded sum of its exact terms; per sum the sum of |term|, for the comparison's bound)"""
    J, e = J.astype(f64), e.astype(f64)
    terms = [J[:, a] * J[:, b] for a, b in TRI] + [J[:, a] * e for a in range(6)] + [e * e]
    sums = np.array([math.fsum(q.tolist()) for q in terms] + [float(len(e))], f64)
    mags = np.array([math.fsum(np.abs(q).tolist()) for q in terms] + [0.0], f64)
    return sums, mags


def np_sums(dst, src, xf, centre):
    """np_row_sums of np_rows"""
    return np_row_sums(*np_rows(dst, src, xf, centre))


def matrix_of(sums):
    A = np.zeros((6, 6))
    for k, (a, b) in enumerate(TRI):
        A[a, b] = A[b, a] = sums[k]
    return A, np.asarray(sums[21:27], f64)


def np_exp(xi):
    """(exp(omega^), V v) of the twist xi = (omega, v)"""
    w, v = np.asarray(xi[:3], f64), np.asarray(xi[3:], f64)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-4:
        A, B, C = 1 - th * th / 6, 0.5 - th * th / 24, 1 / 6 - th * th / 120
    else:
        A, B, C = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + A * W + B * W @ W, (np.eye(3) + B * W + C * W @ W) @ v


def np_step(sums, centre, xf):
    """(the updated transform, xi) or None when A is not positive definite: xf <- T(centre) exp(xi) T(-centre) xf"""
    A, b = matrix_of(sums)
    try:
        np.linalg.cholesky(A)
        xi = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(xi)):
        return None
    E, u = np_exp(xi)
    c = np.asarray(centre, f64)
    return xf_of(E @ xf[:, :3], E @ (xf[:, 3] - c) + c + u), xi


def np_gauss_newton(eval_sums, xf, centre, max_iter, min_pairs, eps_rot, eps_trans):
    """the loop of kf_align_brick_store and kf_map_refine_poses over eval_sums(xf) -> the 29 sums: (xf, verdict, iterations, the last evaluation's sums, the
    last step)"""
    xf = good = np.asarray(xf, f64).reshape(3, 4)
    it, step = 0, np.zeros(6)
    while True:
        sums = eval_sums(xf)
        if sums[28] < max(min_pairs, 1):
            return good, FEW_PAIRS, it, sums, step
        good = xf
        if it >= max_iter:
            return good, ITER_LIMIT, it, sums, step
        nxt = np_step(sums, centre, xf)
        if nxt is None:
            return good, SINGULAR, it, sums, step
        xf, step = nxt
        it += 1
        if np.linalg.norm(step[:3]) <= max(eps_rot, EPS_ROT_MIN) and np.linalg.norm(step[3:]) <= max(eps_trans, EPS_TRANS_MIN):
            return xf, CONVERGED, it, sums, step


def np_align(dst, src, xf, centre, max_iter=25, min_pairs=1000, eps_rot=1e-9, eps_trans=1e-9):
    """kf_align_brick_store's loop over np_sums: (xf, verdict, iterations, the last evaluation's sums, the last step)"""
    return np_gauss_newton(lambda x: np_sums(dst, src, x, centre)[0], xf, centre, max_iter, min_pairs, eps_rot, eps_trans)


def errors(xf, truth, at):
    """(how far the images of the point `at` lie apart, voxels; the angle between the rotations, radians)"""
    from hybkinectfu_amd import posemath
    at = np.asarray(at, f64)
    return (float(np.linalg.norm((xf[:, :3] @ at + xf[:, 3]) - (truth[:, :3] @ at + truth[:, 3]))), posemath.rotation_angle(xf[:, :3], truth[:, :3]))
