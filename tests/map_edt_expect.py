"""The yardstick of the map's distance field (kf_map_distance_field), not collected: include/hybkf.h's definition restated in numpy.  np_classify gives the
class bytes, np_edt the squared distances by the three windowed integer passes (x, then y, then z, each over +-R, values above R^2 cut to FAR after each),
np_brute the O(voxels x sites) minimum the passes are held against (tests/test_map_edt_cpu.py).  dense_classes assembles the classes of a box widened by R
from a dictionary "world brick (x, y, z) -> (tsdf, weight, colour)" as tests/map_query_expect.py describes it -- built window-first by whoever makes it: a
brick of the window stands for itself even where the store holds a copy.  Then the analytic maps and boxes the CPU and the GPU test share, and case_mix,
which counts the kinds of voxel a set must hold for a GPU comparison on it to mean something.  Everything is integers."""
import functools

import numpy as np

import map_query_expect as Q

f32, u8, u16 = np.float32, np.uint8, np.uint16
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
FAR = 0xFFFF
BIG = 1 << 40
KEY_MIN, KEY_MAX = Q.KEY_MIN, Q.KEY_MAX


def np_classify(tsdf, weight, level):
    """the class byte: UNKNOWN where the true weight is not > 0, else FREE where tsdf > level, else OCCUPIED"""
    t, w = np.asarray(tsdf, f32), np.asarray(weight, f32)
    return np.where(w > 0, np.where(t > f32(level), FREE, OCCUPIED), UNKNOWN).astype(u8)


def np_edt(site, R, box):
    """site: bool (nz + 2R, ny + 2R, nx + 2R), the box (nx, ny, nz) widened by R on every side.  Returns uint16 (nz, ny, nx): the squared distance to the
    nearest site where it is <= R^2, else FAR"""
    nx, ny, nz = (int(v) for v in box)
    R = int(R)
    R2 = R * R
    site = np.asarray(site, bool)
    assert site.shape == (nz + 2 * R, ny + 2 * R, nx + 2 * R), (site.shape, box, R)
    d = np.full((nz + 2 * R, ny + 2 * R, nx), BIG, np.int64)         # x pass: the nearest site of the row within +-R, squared (rows without a site stay BIG)
    rows = np.nonzero(site.any(axis=2))
    if len(rows[0]):
        sub = site[rows]
        best = np.full((len(sub), nx), BIG, np.int64)
        for j in range(-R, R + 1):
            best = np.where(sub[:, R + j:R + j + nx], np.minimum(best, j * j), best)
        d[rows] = best
    e = np.full((nz + 2 * R, ny, nx), BIG, np.int64)                 # y pass
    for j in range(-R, R + 1):
        e = np.minimum(e, d[:, R + j:R + j + ny, :] + j * j)
    e[e > R2] = BIG
    f = np.full((nz, ny, nx), BIG, np.int64)                         # z pass
    for j in range(-R, R + 1):
        f = np.minimum(f, e[R + j:R + j + nz] + j * j)
    f[f > R2] = FAR
    return f.astype(u16)


def np_brute(site, R, box, chunk=256):
    """the definition: per voxel of the box the minimum of |s - g|^2 over the sites of the widened region, FAR above R^2"""
    nx, ny, nz = (int(v) for v in box)
    R = int(R)
    s = np.argwhere(np.asarray(site, bool)).astype(np.int64) - R      # (z, y, x) in the box's frame
    g = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    out = np.full(len(g), BIG, np.int64)
    if len(s):
        for i in range(0, len(g), chunk):
            out[i:i + chunk] = ((g[i:i + chunk, None, :] - s[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    out[out > R * R] = FAR
    return out.astype(u16).reshape(nz, ny, nx)


def dense_classes(bricks, lo, dims, R, level):
    """the classes of the box (lo (x, y, z), dims (nx, ny, nz)) widened by R, (nz + 2R, ny + 2R, nx + 2R): UNKNOWN where the dictionary holds no brick or the
    brick coordinate lies outside the key range"""
    lo = np.asarray(lo, np.int64) - int(R)
    n = np.asarray(dims, np.int64) + 2 * int(R)
    out = np.zeros((n[2], n[1], n[0]), u8)
    for k, v in bricks.items():
        if not all(KEY_MIN <= c < KEY_MAX for c in k):
            continue
        o = 8 * np.asarray(k, np.int64) - lo
        a, b = np.maximum(o, 0), np.minimum(o + 8, n)
        if np.any(a >= b):
            continue
        c = np_classify(np.asarray(v[0]).reshape(8, 8, 8), np.asarray(v[1]).reshape(8, 8, 8), level)
        out[a[2]:b[2], a[1]:b[1], a[0]:b[0]] = c[a[2] - o[2]:b[2] - o[2], a[1] - o[1]:b[1] - o[1], a[0] - o[0]:b[0] - o[0]]
    return out


def sites_of(classes, site_mask):
    return np.array([(int(site_mask) >> c) & 1 for c in range(3)], bool)[classes]


def expected(bricks, lo, dims, R, level=0.0, site_mask=1 << OCCUPIED):
    """(dist2 (nz, ny, nx) uint16, cls (nz, ny, nx) uint8) of kf_map_distance_field on the map `bricks`"""
    c = dense_classes(bricks, lo, dims, R, level)
    nx, ny, nz = dims
    return np_edt(sites_of(c, site_mask), R, dims), np.ascontiguousarray(c[R:R + nz, R:R + ny, R:R + nx])


# ---- the analytic maps and boxes -------------------------------------------------------------------------------------------------------------------------
BOX_LO, BOX_DIMS = (-13, 5, -70), (40, 24, 17)                      # negative, not brick-aligned
BOX9_LO, BOX9_DIMS = (-3, 2, -61), (9, 9, 9)                         # for R = 255
# map_query_expect's maps (bricks 0 .. 8) moved, by whole bricks, to where the surface cuts the box's far end and leaves its low corner further than 37
# voxels from it: so that at every radius the set holds voxels on the surface, near it, at R, just beyond R and far (test_map_edt_cpu.py asserts that)
MAP_SHIFT = {"single": (0, 0, 0), "plane": (3, -5, -14), "sphere": (0, 0, -9)}
RADII = (1, 7, 37)
# per R: an offset of squared length R^2 -- every component non-zero where R^2 has such a form (R = 1 has none) -- and one of squared length R^2 + 1
SPECIAL = {1: ((1, 0, 0), (1, 1, 0)), 7: ((2, 3, 6), (3, 4, 5)), 37: ((36, 8, 3), (36, 7, 5)), 255: ((120, 135, 180), (255, 1, 0))}
for _r, (_a, _b) in SPECIAL.items():
    assert sum(v * v for v in _a) == _r * _r and sum(v * v for v in _b) == _r * _r + 1


def _put_site(bricks, g):
    """world voxel g made an occupied voxel (tsdf -0.5, weight 1); a brick made for it is observed free everywhere else"""
    k = tuple(int(v) >> 3 for v in g)
    if k in bricks:
        t, w = np.array(bricks[k][0], f32).reshape(8, 8, 8), np.array(bricks[k][1], f32).reshape(8, 8, 8)
    else:
        t, w = np.ones((8, 8, 8), f32), np.ones((8, 8, 8), f32)
    t[g[2] & 7, g[1] & 7, g[0] & 7], w[g[2] & 7, g[1] & 7, g[0] & 7] = -0.5, 1.0
    bricks[k] = (t, w, None)


def special_sites(lo, dims, R):
    """single sites: at squared distance exactly R^2 from the box's low corner and R^2 + 1 from its high corner, both outside the box and off it on every axis
    the offset has; and two inside it next to the high corner -- further than R from the low one --, on either side of the voxel hi - (gap, 1, 1) at the
    same distance `gap` from it (so the site off the high corner is not the nearest there: case_mix finds the voxels that read FAR by one).  R = 255 goes with a box of 9 voxels, where a
    site inside the box would leave no voxel further than 14 from it: there the pair stands 250 voxels off the high corner along x instead, two voxels apart
    in y, so that the box holds voxels nearer than R, at R and beyond it, and the voxels of the row y = hi - 1 between the two are tied"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(lo, np.int64) + np.asarray(dims, np.int64) - 1
    a, b = SPECIAL[R]
    if R == 255:
        return [lo - np.array(a), hi + np.array(b), hi + np.array([250, 0, 0]), hi + np.array([250, -2, 0])]
    gap = 1 if R == 1 else 2
    return [lo - np.array(a), hi + np.array(b), hi - np.array([0, 1, 1]), hi - np.array([2 * gap, 1, 1])]


@functools.lru_cache(maxsize=None)
def analytic_map(kind, R, lo=BOX_LO, dims=BOX_DIMS):
    """kind: "single" (the special sites alone), "plane" / "sphere" (map_query_expect's map moved over the box, colour dropped, plus the special sites),
    "empty".  (shared: nobody writes into it)"""
    if kind == "empty":
        return {}
    base = {"single": {}, "plane": Q.plane_map(), "sphere": Q.sphere_map()}[kind]
    bricks = {k: (t, w, None) for k, (t, w, c) in Q.shifted(base, MAP_SHIFT[kind]).items()}
    for g in special_sites(lo, dims, R):
        _put_site(bricks, g)
    return bricks


def analytic_sets():
    """(kind, R, lo, dims) of every analytic set the GPU test compares"""
    return [(kind, R, BOX_LO, BOX_DIMS) for kind in ("single", "plane", "sphere") for R in RADII] + [("single", 255, BOX9_LO, BOX9_DIMS)]


def moved_lo(lo, db):
    return tuple(int(v) + 8 * int(d) for v, d in zip(lo, db))


def case_mix(bricks, lo, dims, R, level=0.0, site_mask=1 << OCCUPIED):
    """how many voxels of each kind the set holds: zero (d2 = 0), inside (0 < d2 < R^2), exact (d2 = R^2), far_by_one (the nearest site at R^2 + 1: reads
    FAR), halo (within R^2 only thanks to a site outside the box), diagonal (within R^2, or nearer, only thanks to a site off the box on all three axes),
    tie (two sites at the least distance; looked for in the z slice nz - 2 of the box)"""
    nx, ny, nz = dims
    R2 = R * R
    site = sites_of(dense_classes(bricks, lo, dims, R, level), site_mask)
    d = np_edt(site, R, dims).astype(np.int64)
    wide = np_edt(sites_of(dense_classes(bricks, lo, dims, R + 1, level), site_mask), R + 1, dims).astype(np.int64)
    inner = np.zeros_like(site)
    inner[R:R + nz, R:R + ny, R:R + nx] = site[R:R + nz, R:R + ny, R:R + nx]
    d_in = np_edt(inner, R, dims).astype(np.int64)
    d_in[d_in == FAR] = BIG
    edge = site.copy()                                              # without the sites off the box on all three axes
    for sz in (slice(0, R), slice(R + nz, None)):
        for sy in (slice(0, R), slice(R + ny, None)):
            for sx in (slice(0, R), slice(R + nx, None)):
                edge[sz, sy, sx] = False
    d_edge = np_edt(edge, R, dims).astype(np.int64)
    s = np.argwhere(site).astype(np.int64) - R                       # (z, y, x)
    z = nz - 2                                                       # (special_sites' pair lies in this slice)
    g = np.stack(np.meshgrid([z], np.arange(ny), np.arange(nx), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    ties = 0
    if len(s):
        for i in range(0, len(g), 64):
            q = ((g[i:i + 64, None, :] - s[None, :, :]) ** 2).sum(axis=2)
            m = q.min(axis=1)
            ties += int(np.count_nonzero((m > 0) & (m <= R2) & ((q == m[:, None]).sum(axis=1) >= 2)))
    return dict(zero=int(np.count_nonzero(d == 0)), inside=int(np.count_nonzero((d > 0) & (d < R2))), exact=int(np.count_nonzero(d == R2)),
                far_by_one=int(np.count_nonzero((d == FAR) & (wide == R2 + 1))), halo=int(np.count_nonzero((d != FAR) & (d < d_in))),
                diagonal=int(np.count_nonzero((d != FAR) & (d < np.where(d_edge == FAR, BIG, d_edge)))), tie=ties)
