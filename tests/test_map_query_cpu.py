"""CPU-only: the yardstick of the map queries and the case mix of the GPU test, checked before any GPU is involved.  map_query_expect.np_sample / np_cast
restate kf_map_sample / kf_map_cast_rays in numpy; here they are held against what is known in closed form on the analytic maps, and the point and ray
sets tests/test_gpu_map_query.py uses are shown to hold enough of every kind -- so that test cannot pass by comparing zeros."""
import functools

import numpy as np

import map_query_expect as E

f32 = np.float32


@functools.lru_cache(maxsize=None)
def plane():
    return E.MapIndex(E.plane_map())


@functools.lru_cache(maxsize=None)
def sphere():
    return E.MapIndex(E.sphere_map())


@functools.lru_cache(maxsize=None)
def sphere_cast():
    return E.np_cast(sphere(), *E.sphere_rays(), E.STEP)


@functools.lru_cache(maxsize=None)
def sphere_sampled():
    return E.np_sample(sphere(), E.sphere_points(), detail=True)


def test_a_voxel_centre_returns_the_voxel_verbatim():
    """all eight corners must be observed, the fractions are 0: the value is corner 0's, the weight the least of the eight"""
    bricks = E.plane_map()
    key = sorted(bricks)[len(bricks) // 2]
    t, w, c = bricks[key]
    z, y, x = np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij")
    g = np.stack([8 * key[0] + x, 8 * key[1] + y, 8 * key[2] + z], axis=-1).reshape(-1, 3)
    s = E.np_sample(bricks, g + 0.5)
    assert s["observed"].all()
    assert np.array_equal(s["tsdf"].view(np.uint32), t[:7, :7, :7].reshape(-1).view(np.uint32))
    assert np.array_equal(s["color"][:, :3], c[:7, :7, :7].reshape(-1, 3)) and not s["color"][:, 3].any()
    w8 = np.min([w[dz:dz + 7, dy:dy + 7, dx:dx + 7] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], axis=0)
    assert np.array_equal(s["weight"], w8.reshape(-1))
    # one brick alone: a voxel whose neighbours nobody holds is unobserved, and reads zeros
    alone = E.np_sample({key: bricks[key]}, np.array([[8 * key[0] + 7.5, 8 * key[1] + 3.5, 8 * key[2] + 3.5]]))
    assert not alone["observed"][0] and alone["tsdf"][0] == 0 and alone["weight"][0] == 0 and not alone["color"].any() and not alone["grad"].any()


def test_plane_rays_hit_the_analytic_intersection():
    """256 rays, coordinates below 2^9 voxels: fp32 resolves 6e-5 there and the chain is a handful of rounded operations; a half-voxel convention error
    would be 50 times the bound"""
    o, d, t0, t1 = E.plane_rays()
    assert len(o) >= 200 and np.abs(o).max() < 512
    r = E.np_cast(plane(), o, d, t0, t1, E.STEP)
    assert (r["status"] == E.HIT).all()
    dd = d.astype(np.float64)
    t_true = (E.PLANE_D - o @ E.PLANE_N) / (dd @ E.PLANE_N)
    err = np.abs(r["t"] - t_true) * np.linalg.norm(dd, axis=1)
    print("plane: worst |t - t*| in voxels", err.max())
    assert err.max() < 0.01
    cos = np.abs(r["normal"].astype(np.float64) @ E.PLANE_N)
    assert cos.min() > 1 - 1e-5 and np.all(r["normal"].astype(np.float64) @ E.PLANE_N > 0)     # out of the surface: towards growing tsdf


def test_plane_gradient_is_the_normal_over_the_truncation():
    rng = np.random.default_rng(3)
    p = np.array([32.0, 32.0, 32.0]) + rng.uniform(-12, 12, (512, 3))
    p -= ((p @ E.PLANE_N - E.PLANE_D)[:, None] - rng.uniform(-2, 2, (512, 1))) * E.PLANE_N      # within 2 voxels of the plane: every corner inside the band
    s = E.np_sample(plane(), p)
    assert s["observed"].all()
    assert np.abs(s["grad"] - E.PLANE_N / E.TRUNC).max() < 1e-4
    assert np.abs(s["tsdf"] - (p @ E.PLANE_N - E.PLANE_D) / E.TRUNC).max() < 1e-4


def test_the_sphere_ray_set_holds_every_kind():
    o, d, t0, t1 = E.sphere_rays()
    r = sphere_cast()
    n_hit, n_miss = np.count_nonzero(r["status"] == E.HIT), np.count_nonzero(r["status"] == E.MISS)
    n_b1, n_b2 = np.count_nonzero(r["kind"] == 1), np.count_nonzero(r["kind"] == 2)
    n_zero = np.count_nonzero(np.any(d == 0, axis=1))
    print("sphere rays: hit", n_hit, "miss", n_miss, "broken corner", n_b1, "broken hit", n_b2, "zero component", n_zero)
    assert len(o) == 2048
    assert n_hit >= 1024 and n_miss >= 64 and n_b1 >= 16 and n_b2 >= 16 and n_zero >= 32
    assert np.count_nonzero((r["status"] == E.HIT) & np.any(d == 0, axis=1)) >= 32
    assert np.all((r["kind"] != 0) == (r["status"] == E.BROKEN))
    hit = r["status"] == E.HIT
    assert r["t"][hit].min() >= 8                                 # what makes the far-key cases exact (map_query_expect's docstring)
    # the lattices that make a moved map give the same bytes
    assert np.array_equal(o * 2 ** 20, np.round(o * 2 ** 20)) and np.array_equal(d * 256, np.round(d * 256)) and np.array_equal(t0 * 16, np.round(t0 * 16))
    # non-hits are zeros; hits lie on the sphere
    assert not r["t"][~hit].any() and not r["normal"][~hit].any() and not r["color"][~hit].any() and not r["weight"][~hit].any()
    at = o[hit] + r["t"][hit, None].astype(np.float64) * d[hit].astype(np.float64)
    assert np.abs(np.linalg.norm(at - E.SPHERE_C, axis=1) - E.SPHERE_R).max() < 0.1


def test_the_sphere_point_set_holds_every_kind():
    p = E.sphere_points()
    s = sphere_sampled()
    obs = s["observed"]
    n_obs, n_un = np.count_nonzero(obs), np.count_nonzero(~obs)
    n_zero, n_span = np.count_nonzero(s["zero_frac"] & obs), np.count_nonzero(s["span"] & obs)
    print("sphere points: observed", n_obs, "unobserved", n_un, "observed with a zero fraction", n_zero, "observed across bricks", n_span)
    assert len(p) == 4096
    assert n_obs >= 1024 and n_un >= 256 and n_zero >= 256 and n_span >= 256
    assert np.count_nonzero(s["color"][obs, :3]) > 1000 and np.count_nonzero(s["grad"][obs]) > 3000
    body = p[:-E.N_ODD]
    assert np.array_equal(body * 2 ** 20, np.round(body * 2 ** 20))
    assert not s["observed"][-E.N_ODD:-5].any()                   # not finite, beyond the range, at its ends


def test_moving_map_and_queries_by_whole_bricks_changes_nothing():
    for db in (E.FAR, (-3, 7, 100000)):
        far = E.MapIndex(E.shifted(E.sphere_map(), db))
        p = E.sphere_points()[:-E.N_ODD]
        a, b = E.np_sample(sphere(), p), E.np_sample(far, E.moved(p, db))
        for k in ("tsdf", "weight", "grad", "color"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (db, k)
        o, d, t0, t1 = E.sphere_rays()
        a, b = sphere_cast(), E.np_cast(far, E.moved(o, db), d, t0, t1, E.STEP)
        for k in ("status", "t", "normal", "color", "weight"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (db, k)


def test_the_march_obeys_t_max_and_max_steps():
    o, d, t0, t1 = E.sphere_rays()
    full = sphere_cast()
    hit = np.flatnonzero(full["status"] == E.HIT)[:64]
    k_hit = np.ceil((full["t"][hit] - t0[hit]) / f32(E.STEP)).astype(int)      # the crossing sample's index
    few = E.np_cast(sphere(), o[hit], d[hit], t0[hit], t1[hit], E.STEP, max_steps=int(k_hit.min()))
    assert (few["status"] == E.MISS).all()
    enough = E.np_cast(sphere(), o[hit], d[hit], t0[hit], t1[hit], E.STEP, max_steps=int(k_hit.max()) + 1)
    assert np.array_equal(enough["t"], full["t"][hit])
    short = E.np_cast(sphere(), o[hit], d[hit], t0[hit], full["t"][hit] - f32(E.STEP), E.STEP)
    assert (short["status"] == E.MISS).all()
