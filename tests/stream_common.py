"""Shared by test_gpu_mc_region.py and test_gpu_stream_mesh.py: the fused box-and-sphere scene at 64 @ 2.0 m and 72 @ 2.25 m (cell = 1 / 32, so
(float)origin * cell is exact in numpy fp32; 72 gives 9 bricks per axis: every table has a ragged end), fused ONCE per (resolution, colour) and
handed to every test as planes + pose; the adversarial volume of test_gpu_mcubes.py restated; and the masked-volume construction that states what
a region extraction must return without running it: a cell's triangles depend on its 27 voxels alone, so kf_marching_cubes on a volume that is
zero (never observed) outside voxels [lo - 1, hi + 1) emits exactly the triangles of the cells lo <= (x, y, z) < hi, in the same order."""
import numpy as np

from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

P = S.STOCK
CAM = (160, 120, 79.5, 59.5, 131.25, 131.25)
RGB_CAM = S.vga_camera()
f32 = np.float32
SIZES = {40: 1.25, 64: 2.0, 72: 2.25}                             # cell = 1 / 32 each
GATE = 2.5
MAX_TRI = 300000


def thr_of(res):
    return 300 * SIZES[res] / res                                 # MeshGeneratorMarchingcube.cpp:23-29


def bgr(k):
    y, x = np.mgrid[0:RGB_CAM[1], 0:RGB_CAM[0]]
    return np.stack([(x * 3 + k * 7) % 256, (y * 5 + x) % 256, (x + 2 * y + 31 * k) % 256], axis=-1).astype(np.uint8)


_FRAMES = {}


def frame(k, size):
    if (k, size) not in _FRAMES:
        _FRAMES[(k, size)] = S.render_depth_mm(S.trajectory_pose(k, size), CAM, size)
    return _FRAMES[(k, size)]


def make_ctx(res, color=False, max_triangles=MAX_TRI, **kw):
    if color:
        kw["rgb_cam"] = K.camera(*RGB_CAM)
    return K.Context(K.camera(*CAM), res, SIZES[res], P["volume_max_weight"], levels=3, max_triangles=max_triangles, has_color=color, **kw)


def raycast(ctx, color=False):
    ctx.raycast(None, 0.7 * 5 * ctx.size / ctx.res, P["depth_trunc_min"], P["depth_trunc_max"], has_color=color)


def run_frame(ctx, k, color=False):
    size = ctx.size
    ctx.upload_depth_mm(frame(k, size))
    if color:
        ctx.upload_rgb(bgr(k))
    ctx.preprocess(P["depth_trunc_min"], P["depth_trunc_max"], P["filter_sigma_pixel"], P["filter_sigma_depth"])
    ctx.icp_track(k, P["icp_thre_dist"], P["icp_thre_sin_angle"], P["camera_shake_dist"], P["camera_shake_angle"])
    ctx.integrate(None, 5 * size / ctx.res, GATE, has_color=color, angle_weight=color)
    raycast(ctx, color)
    ok, pose, _, _ = ctx.track_result()
    return ok, pose


def fuse(ctx, frames, color=False):
    ctx.set_pose(S.pose0(ctx.size))
    for k in frames:
        ok, _ = run_frame(ctx, k, color)
        assert ok, k


def planes(ctx, color=False):
    return ctx.download_volume(color=True) if color else ctx.download_volume() + (None,)


_FUSED = {}


def fused(res, color=False):
    """(tsdf, weight, colour or None, pose) of the scene after 5 fused frames; computed once, never modified"""
    key = (res, color)
    if key not in _FUSED:
        ctx = make_ctx(res, color, max_triangles=0)
        fuse(ctx, range(5), color)
        t, w, c = planes(ctx, color)
        pose = ctx.track_result()[1]
        ctx.close()
        assert np.count_nonzero(w) > 1000 and np.any(t < 0)
        for a in (t, w, c):
            if a is not None:
                a.setflags(write=False)
        _FUSED[key] = (t, w, c, pose)
    return _FUSED[key]


def ctx_with(res, t, w, c=None, pose=None, max_triangles=MAX_TRI):
    """a fresh context that holds the given planes (and pose)"""
    ctx = make_ctx(res, c is not None, max_triangles)
    ctx.upload_volume(t, w, c)
    if pose is not None:
        ctx.set_pose(pose)
    return ctx


def scene_ctx(res, color=False, max_triangles=MAX_TRI):
    t, w, c, pose = fused(res, color)
    return ctx_with(res, t, w, c, pose, max_triangles)


def smooth_field(res, rng, waves=4):
    z, y, x = np.meshgrid(*(np.arange(res, dtype=np.float32),) * 3, indexing="ij")
    f = np.zeros((res, res, res), np.float32)
    for _ in range(waves):
        k = rng.uniform(0.15, 0.9, 3).astype(np.float32)
        ph = rng.uniform(0, 6.28, 3).astype(np.float32)
        f += np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
    return (f / waves).astype(np.float32)


def stress_volume(res, seed):
    """test_gpu_mcubes.py's adversarial volume: holes, negatives that round to nothing, -0.0 / +0.0, solid regions, surface on the rim"""
    rng = np.random.default_rng(seed)
    t = smooth_field(res, rng)
    w = np.ones_like(t) * 3.0
    q = res // 4
    w[rng.random(t.shape) < 0.02] = 0.0
    w[q:q + 5, 2:9, :] = 0.0
    t[:q, :q, :q] = -0.25
    t[:3, q:2 * q, q:2 * q] = -1e-20
    t[3:6, q:2 * q, q:2 * q] = -1e-38
    t[6:8, q:2 * q, q:2 * q] = np.float32(-1e-45)
    t[2 * q:2 * q + 4, :q, :] = np.where(rng.random((4, q, res)) < 0.5, np.float32(-0.0), np.float32(0.0))
    t[-q:, -q:, -q:] = np.abs(t[-q:, -q:, -q:]) + 0.01
    tiny = rng.random(t.shape) < 0.01
    t[tiny] = (rng.choice(np.array([-1e-19, -3e-18, -1e-17, 1e-19], np.float32), int(tiny.sum())))
    return t.astype(np.float32), w.astype(np.float32)


def stress_color(res, seed):
    return np.random.default_rng(seed + 77).integers(0, 256, (res, res, res, 3), dtype=np.uint8)


def clamp_box(lo, hi, res):
    return [min(max(int(v), 0), res) for v in lo], [min(max(int(v), 0), res) for v in hi]


def masked(a, lo, hi):
    """a (planes in (z, y, x[, c]) order) with everything outside voxels [lo - 1, hi + 1) zeroed; lo / hi in (x, y, z), clamped cells"""
    out = np.zeros_like(a)
    R = a.shape[0]
    sl = tuple(slice(max(lo[k] - 1, 0), min(hi[k] + 1, R)) for k in (2, 1, 0))
    out[sl] = a[sl]
    return out


def masked_soup(res, t, w, c, lo, hi, thr, max_triangles=MAX_TRI):
    """what kf_marching_cubes_region(lo, hi) must append: the EXISTING whole-volume extraction of a fresh context holding the masked volume"""
    lo, hi = clamp_box(lo, hi, res)
    ctx = ctx_with(res, masked(t, lo, hi), masked(w, lo, hi), masked(c, lo, hi) if c is not None else None, max_triangles=max_triangles)
    ctx.marching_cubes(thr, has_color=c is not None)
    out = ctx.triangles()
    ctx.close()
    assert len(out) < max_triangles
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def words(tris):
    return np.ascontiguousarray(tris).view(np.uint32).reshape(-1, 18)


def sorted_words(tris):
    w = words(tris)
    return w[np.lexsort(w.T[::-1])] if len(w) else w


def to_world(tris, origin, cell):
    """+ (float)origin * cell on every position, numpy fp32: one multiply, one add"""
    out = np.array(tris, copy=True)
    off = np.array([f32(origin[i]) * f32(cell) for i in range(3)], f32)
    out["v"]["pos"] = out["v"]["pos"] + off
    return out


def np_shift(a, d):
    """out[z, y, x] = a[z + dz, y + dy, x + dx] inside the volume, zero elsewhere"""
    out = np.zeros_like(a)
    R = a.shape[0]
    sl_dst, sl_src = [], []
    for s in (d[2], d[1], d[0]):
        if abs(s) >= R:
            return out
        sl_dst.append(slice(max(0, -s), R - max(0, s)))
        sl_src.append(slice(max(0, s), R - max(0, -s)))
    out[tuple(sl_dst)] = a[tuple(sl_src)]
    return out


def is_subsequence(part, whole):
    """every triangle of `part` appears in `whole`, in the same order"""
    pw, ww = words(part), words(whole)
    keys = [r.tobytes() for r in ww]
    j = 0
    for r in pw:
        b = r.tobytes()
        while j < len(keys) and keys[j] != b:
            j += 1
        if j == len(keys):
            return False
        j += 1
    return True
