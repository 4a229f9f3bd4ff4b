"""The yardstick of the map queries (kf_map_sample, kf_map_cast_rays), not collected: np_sample and np_cast restate include/hybkf.h's definition in numpy
float32 / float64, operation for operation, over a dictionary "world brick (x, y, z) -> (tsdf, weight, colour)" -- each brick (8, 8, 8) in (z, y, x) order,
colour (8, 8, 8, 3) or None -- built window-first by whoever makes it: a brick of the window stands for itself even where the store holds a copy.
Then the analytic maps (truncation 4 voxels, tsdf clamped to +-1, only the bricks that meet the band) and the point and ray sets the CPU and the GPU test
share.  Every generated coordinate is a multiple of 2^-20, every direction component a multiple of 2^-8 and every t_min a multiple of 2^-4 with hits beyond
t = 8, so that origin + (double)(t * dir) is exact at the origin AND 2^23 voxels away: a map moved by whole bricks gives the same bytes."""
import functools

import numpy as np

f32, f64, u8 = np.float32, np.float64, np.uint8
LIMIT = float(1 << 23)                                           # positions beyond +-2^23 voxels read unobserved
KEY_MIN, KEY_MAX = -(1 << 20), 1 << 20                            # the key range in bricks
MISS, HIT, BROKEN = 0, 1, 2
TRUNC = 4.0                                                       # the analytic maps' truncation, voxels
STEP = 0.75                                                       # the march's step on the analytic maps
FAR = (2 ** 20 - 16, -(2 ** 20 - 8), 5)                           # the far-key offset, bricks


def _pack(b):
    b = np.asarray(b, np.int64)
    return (b[..., 0] - KEY_MIN) | ((b[..., 1] - KEY_MIN) << 21) | ((b[..., 2] - KEY_MIN) << 42)


class MapIndex:
    """the dictionary as sorted arrays, for vectorised look-ups"""

    def __init__(self, bricks):
        keys = np.array(sorted(bricks), np.int64).reshape(-1, 3)
        order = np.argsort(_pack(keys)) if len(keys) else np.zeros(0, np.int64)
        keys = keys[order]
        self.keys = keys                                          # row i of the planes belongs to keys[i]
        self.packed = _pack(keys) if len(keys) else np.zeros(0, np.int64)
        n = len(keys)
        self.t, self.w, self.c = np.zeros((n + 1, 512), f32), np.zeros((n + 1, 512), f32), np.zeros((n + 1, 512, 3), u8)   # row n: nobody
        for i, k in enumerate(map(tuple, keys)):
            t, w, c = bricks[k]
            self.t[i], self.w[i] = np.asarray(t, f32).reshape(512), np.asarray(w, f32).reshape(512)
            if c is not None:
                self.c[i] = np.asarray(c, u8).reshape(512, 3)

    def voxel(self, g, valid):
        """world voxels g (n, 3) int64 -> (tsdf, weight, colour, slot): a voxel whose weight is not > 0, or that nobody holds, reads (0, 0, 0)"""
        b = g >> 3                                                # (floors)
        valid = valid & np.all((b >= KEY_MIN) & (b < KEY_MAX), axis=1)
        key = _pack(np.where(valid[:, None], b, 0))
        n = len(self.packed)
        i = np.minimum(np.searchsorted(self.packed, key), max(n - 1, 0))
        found = valid & (self.packed[i] == key) if n else np.zeros(len(g), bool)
        i = np.where(found, i, n)
        off = ((g[:, 2] & 7) << 6) | ((g[:, 1] & 7) << 3) | (g[:, 0] & 7)
        w = self.w[i, off]
        obs = found & (w > 0)
        return np.where(obs, self.t[i, off], f32(0)), np.where(obs, w, f32(0)), np.where(obs[:, None], self.c[i, off], u8(0)), np.where(found, i, -1)


def _index(m):
    return m if isinstance(m, MapIndex) else MapIndex(m)


def _lerp(a, b, f):
    return a + f * (b - a)


def np_sample(m, pos, detail=False):
    """kf_map_sample: dict of tsdf (n,), weight (n,), grad (n, 3), color (n, 4), observed (n,) bool; detail adds zero_frac and span (corners in more than
    one brick) and slots (n, 8): the row of MapIndex.keys each corner was read from, -1 where nobody holds it"""
    m = _index(m)
    pos = np.asarray(pos, f64).reshape(-1, 3)
    n = len(pos)
    with np.errstate(invalid="ignore"):
        inside = np.all(np.abs(pos) <= LIMIT, axis=1)             # (NaN: False)
    p = np.where(inside[:, None], pos, 0.0)
    u = p - 0.5
    fl = np.floor(u)
    f = (u - fl).astype(f32)                                      # the difference is exact: one rounding
    base = fl.astype(np.int64)
    v, w, c, slot = [None] * 8, [None] * 8, [None] * 8, [None] * 8
    for k in range(8):                                            # corner k: x from bit 0, y from bit 1, z from bit 2
        v[k], w[k], c[k], slot[k] = m.voxel(base + np.array([k & 1, (k >> 1) & 1, k >> 2], np.int64), inside)
    ok = inside.copy()
    wmin = w[0]
    for k in range(8):
        ok &= w[k] > 0
        wmin = np.minimum(wmin, w[k])
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    a0, a1, a2, a3 = _lerp(v[0], v[1], fx), _lerp(v[2], v[3], fx), _lerp(v[4], v[5], fx), _lerp(v[6], v[7], fx)
    b0, b1 = _lerp(a0, a1, fy), _lerp(a2, a3, fy)
    tsdf = _lerp(b0, b1, fz)
    d0, d1, d2, d3 = v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6]
    gx = _lerp(_lerp(d0, d1, fy), _lerp(d2, d3, fy), fz)
    gy = _lerp(a1 - a0, a3 - a2, fz)
    gz = b1 - b0
    one = f32(1)
    ia, ib, ic = one - fx, one - fy, one - fz
    acc = None
    for j in range(8):                                            # interpolateColor's corner j: x from bit 2, y from bit 1, z from bit 0
        cj = c[(j >> 2) | (j & 2) | ((j & 1) << 2)].astype(f32)
        wa, wb, wc = (fx if j >> 2 else ia), (fy if (j >> 1) & 1 else ib), (fz if j & 1 else ic)
        t = cj * wa[:, None] * wb[:, None] * wc[:, None]
        acc = t if j == 0 else acc + t
    color = np.zeros((n, 4), u8)
    color[:, :3] = np.where(ok[:, None], acc, f32(0)).astype(np.int32).astype(u8)   # truncated
    z = f32(0)
    out = dict(tsdf=np.where(ok, tsdf, z), weight=np.where(ok, wmin, z), grad=np.where(ok[:, None], np.stack([gx, gy, gz], axis=1), z), color=color, observed=ok)
    assert out["tsdf"].dtype == f32 and out["grad"].dtype == f32 and out["weight"].dtype == f32
    if detail:
        out["zero_frac"] = np.any(f == 0, axis=1)
        out["span"] = np.any((base & 7) == 7, axis=1)
        s = np.stack(slot, axis=1)
        out["slots"] = s
    return out


def _nearest(m, pos):
    with np.errstate(invalid="ignore"):
        inside = np.all(np.abs(pos) <= LIMIT, axis=1)
    g = np.floor(np.where(inside[:, None], pos, 0.0)).astype(np.int64)
    return m.voxel(g, inside)[0]


def np_cast(m, origin, dirs, tmin, tmax, step, max_steps=1 << 24):
    """kf_map_cast_rays: dict of status (n,) u8, t (n,), normal (n, 3), color (n, 4), weight (n,), and kind (n,): 0 none, 1 a BROKEN ray with an unobserved
    corner at sample k - 1 or k, 2 a BROKEN ray whose hit sample is unobserved or has no gradient"""
    m = _index(m)
    origin, dirs = np.asarray(origin, f64).reshape(-1, 3), np.asarray(dirs, f32).reshape(-1, 3)
    n = len(origin)
    tmin, tmax = np.broadcast_to(np.asarray(tmin, f32), (n,)), np.broadcast_to(np.asarray(tmax, f32), (n,))
    step = f32(step)
    assert np.isfinite(step) and step > 0 and 1 <= max_steps <= 1 << 24
    out = dict(status=np.zeros(n, u8), t=np.zeros(n, f32), normal=np.zeros((n, 3), f32), color=np.zeros((n, 4), u8), weight=np.zeros(n, f32), kind=np.zeros(n, u8))
    last = np.zeros(n, f32)
    act = np.arange(n)
    k = 0
    with np.errstate(all="ignore"):
        while k < max_steps and len(act):
            tk = tmin[act] + f32(k) * step
            act = act[tk < tmax[act]]
            if not len(act):
                break
            tk = tmin[act] + f32(k) * step
            pos = origin[act] + (tk[:, None] * dirs[act]).astype(f64)      # the product in fp32, the sum in fp64
            s = _nearest(m, pos)
            cross = (last[act] > 0) & (s < 0)
            if cross.any():
                i = act[cross]
                tk_i = tk[cross]
                tl = tmin[i] + f32(k - 1) * step
                s1 = np_sample(m, pos[cross])
                s0 = np_sample(m, origin[i] + (tl[:, None] * dirs[i]).astype(f64))
                ftdt, ft = s1["tsdf"], s0["tsdf"]
                alpha = tk_i - step * ftdt / (ftdt - ft)
                assert alpha.dtype == f32
                sh = np_sample(m, origin[i] + (alpha[:, None] * dirs[i]).astype(f64))
                g = sh["grad"]
                ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
                both = s0["observed"] & s1["observed"]
                hit = both & sh["observed"] & (ln >= f32(1e-8))
                out["status"][i] = np.where(hit, HIT, BROKEN)
                out["kind"][i] = np.where(hit, 0, np.where(both, 2, 1))
                out["t"][i] = np.where(hit, alpha, f32(0))
                out["normal"][i] = np.where(hit[:, None], g / ln[:, None], f32(0))
                out["color"][i] = np.where(hit[:, None], sh["color"], u8(0))
                out["weight"][i] = np.where(hit, sh["weight"], f32(0))
            last[act] = s
            act = act[~cross]
            k += 1
    return out


# ---- analytic maps ---------------------------------------------------------------------------------------------------------------------------------
def _analytic(sd_of, lo, hi, punched=()):
    """bricks [lo, hi)^3 that meet the band of the signed distance sd_of(centres (..., 3)) in voxels; weights 1..7 and colours from the coordinates"""
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    punched = set(map(tuple, punched))
    bricks = {}
    for bz in range(lo, hi):
        for by in range(lo, hi):
            for bx in range(lo, hi):
                g = np.stack([8 * bx + x, 8 * by + y, 8 * bz + z], axis=-1)
                sd = sd_of(g + 0.5) / TRUNC
                if not np.any(np.abs(sd) < 1):
                    continue
                w = (1 + (g[..., 0] + 2 * g[..., 1] + 3 * g[..., 2]) % 7).astype(f32)
                c = np.stack([(7 * g[..., 0] + 3) & 255, (13 * g[..., 1] + 5) & 255, (29 * g[..., 2] + 11) & 255], axis=-1).astype(u8)
                for p in punched:
                    if (p[0] >> 3, p[1] >> 3, p[2] >> 3) == (bx, by, bz):
                        w[p[2] & 7, p[1] & 7, p[0] & 7] = 0
                bricks[(bx, by, bz)] = (np.clip(sd, -1, 1).astype(f32), w, c)
    return bricks


PLANE_N = np.array([0.48, -0.6, 0.64])                            # a unit normal, oblique
PLANE_D = float(PLANE_N @ np.array([32.0, 32.0, 32.0])) + 0.3137  # n . p = d; n . centre is a multiple of 0.02: no voxel centre lies on the plane, none reads 0


def plane_map():
    return _analytic(lambda p: p @ PLANE_N - PLANE_D, 0, 8)


SPHERE_C = np.array([33.3, 30.7, 31.9])
SPHERE_R = 20.0


@functools.lru_cache(maxsize=None)
def sphere_punched():
    """voxels within 1.5 voxels of the sphere's surface on the side x > centre + 6, one in six of them: weight 0"""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij"), axis=-1).reshape(-1, 3)
    d = np.linalg.norm(g + 0.5 - SPHERE_C, axis=1) - SPHERE_R
    near = g[(np.abs(d) < 1.5) & (g[:, 0] + 0.5 > SPHERE_C[0] + 6)]
    return near[rng.random(len(near)) < 1 / 6]


@functools.lru_cache(maxsize=None)
def sphere_map():
    """(shared: nobody writes into it)"""
    return _analytic(lambda p: np.linalg.norm(p - SPHERE_C, axis=-1) - SPHERE_R, 0, 8, sphere_punched())


def shifted(bricks, db):
    return {(k[0] + db[0], k[1] + db[1], k[2] + db[2]): v for k, v in bricks.items()}


def _q(a, bits):
    return np.round(np.asarray(a, f64) * 2.0 ** bits) / 2.0 ** bits


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rays(origin, target, tmin, tmax):
    """rays from origin towards target: origin on the 2^-20 lattice, the direction (about unit length) on the 2^-8 lattice, t_min on the 2^-4 lattice"""
    origin = _q(origin, 20)
    d = _q(_unit(np.asarray(target, f64) - origin), 8).astype(f32)
    n = len(origin)
    return origin, d, _q(np.broadcast_to(tmin, (n,)), 4).astype(f32), np.broadcast_to(np.asarray(tmax, f32), (n,)).copy()


def plane_rays(n=256):
    """rays from the positive side onto the plane's middle, coordinates below 2^9"""
    rng = np.random.default_rng(11)
    on = np.array([32.0, 32.0, 32.0]) + rng.uniform(-14, 14, (n, 3))
    on -= ((on @ PLANE_N - PLANE_D)[:, None]) * PLANE_N            # projected onto the plane
    on = on[np.all((on > 10) & (on < 54), axis=1)]
    away = _unit(PLANE_N + rng.uniform(-0.5, 0.5, (len(on), 3)))
    return _rays(on + away * rng.uniform(12, 20, (len(on), 1)), on, 0.0, 60.0)


@functools.lru_cache(maxsize=None)
def sphere_rays():
    """2 048 rays: aimed at the unpunched side (some with a zero direction component, some that end early), tangent and outside, starting inside, through
    the punched patch"""
    rng = np.random.default_rng(23)

    def on_sphere(n, x_sign):
        v = _unit(rng.normal(size=(n, 3)))
        v[:, 0] = x_sign * np.abs(v[:, 0])
        return v
    parts = []
    v = on_sphere(1200, -1)                                        # aimed: from 16..24 voxels above the surface, onto it, a little askew
    tgt = SPHERE_C + SPHERE_R * v
    org = SPHERE_C + (SPHERE_R + rng.uniform(16, 24, (1200, 1))) * _unit(v + rng.uniform(-0.3, 0.3, (1200, 3)))
    parts.append(_rays(org, tgt, rng.uniform(0, 4, 1200), np.where(np.arange(1200) % 10 == 0, 9.0, 70.0)))
    v = on_sphere(96, -1)                                          # a zero direction component: origin and target share a coordinate
    tgt = _q(SPHERE_C + (SPHERE_R - 2) * v, 20)
    org = tgt + 30 * _unit(v + rng.uniform(-0.2, 0.2, (96, 3)))
    ax = np.arange(96) % 3
    org[np.arange(96), ax] = tgt[np.arange(96), ax]
    parts.append(_rays(org, tgt, 0.0, 70.0))
    v = _unit(rng.normal(size=(256, 3)))                           # tangent and outside: the closest approach 20.5 .. 30 voxels from the centre
    side = _unit(np.cross(v, rng.normal(size=(256, 3))))
    near = SPHERE_C + v * rng.uniform(20.5, 30, (256, 1))
    parts.append(_rays(near - 35 * side, near, 0.0, 70.0))
    parts.append(_rays(SPHERE_C + rng.uniform(-8, 8, (96, 3)), SPHERE_C + 40 * _unit(rng.normal(size=(96, 3))), 0.0, 70.0))   # starting inside
    # through the punched patch: aimed at and beside punched voxels.  A crossing whose two samples are observed while the hit between them is not needs
    # the hit in a cell of its own, with a punched corner that neither sample's cell has: about one ray in a hundred.  So 400 rays are chosen from a
    # pool of 6 000 by what the restatement makes of them -- up to 48 of that kind, then the first of the others
    pv = sphere_punched()
    pick = pv[rng.integers(0, len(pv), 6000)] + 0.5 + rng.uniform(-1.2, 1.2, (6000, 3))
    org = SPHERE_C + (SPHERE_R + rng.uniform(16, 24, (6000, 1))) * _unit(pick - SPHERE_C + rng.uniform(-4, 4, (6000, 3)))
    pool = _rays(org, pick, 0.0, 70.0)
    kind = np_cast(sphere_map(), *pool, STEP)["kind"]
    rare = np.flatnonzero(kind == 2)[:48]
    sel = np.sort(np.concatenate([rare, np.flatnonzero(kind != 2)[:400 - len(rare)]]))
    parts.append(tuple(a[sel] for a in pool))
    o, d, t0, t1 = (np.concatenate([p[i] for p in parts]) for i in range(4))
    assert len(o) == 2048
    return o, d, t0, t1


def sphere_points():
    """4 096 points: near the surface, anywhere in the box, on voxel centres, next to brick borders, around the punched patch, and a few that are not finite or
    lie beyond the key range"""
    rng = np.random.default_rng(31)

    def near_surface(n, spread=3.0):
        return SPHERE_C + (SPHERE_R + rng.uniform(-spread, spread, (n, 1))) * _unit(rng.normal(size=(n, 3)))
    a = near_surface(2048)
    b = rng.uniform(-4, 68, (512, 3))
    c = near_surface(512)                                          # a zero fraction: one, two or three coordinates on a voxel centre
    for i in range(512):
        for ax in range(1 + i % 3):
            c[i, (i + ax) % 3] = np.floor(c[i, (i + ax) % 3]) + 0.5
    d = near_surface(512, 2.0)                                     # corners in more than one brick: one coordinate in [8 j + 7.5, 8 j + 8.5)
    ax = np.arange(512) % 3
    d[np.arange(512), ax] = np.round((d[np.arange(512), ax] - 7.5) / 8) * 8 + 7.5 + rng.uniform(0, 1, 512) * (1 - 2.0 ** -19)
    pv = sphere_punched()
    e = pv[rng.integers(0, len(pv), 496)] + 0.5 + rng.uniform(-1.5, 1.5, (496, 3))
    e[:64] = pv[:64] + 0.5                                         # the punched voxels' own centres
    pts = _q(np.concatenate([a, b, c, d, e]), 20)
    odd = np.array([[np.nan, 30, 30], [30, np.inf, 30], [30, 30, -np.inf], [1e30, 30, 30], [30, -1e30, 30], [LIMIT, 30, 30], [30, -LIMIT, 30], [LIMIT + 1, 30, 30],
                    [30, 30, -LIMIT - 1], [LIMIT - 0.25, 30, 30], [30, -LIMIT + 0.25, 30], [53.5, 30.5, 31.5], [13.5, 30.5, 31.5], [0.5, 0.5, 0.5], [-0.5, 63.5, 1e-9],
                    [33.5, 30.5, 31.5]])
    pts = np.concatenate([pts, odd])
    assert len(pts) == 4096
    return pts


N_ODD = 16                                                        # the last points of sphere_points(): not moved with the map by the far-key cases


def moved(points, db):
    """points moved by db bricks: exact, the coordinates are on the 2^-20 lattice"""
    return np.asarray(points, f64) + 8.0 * np.asarray(db, f64)
