"""The three byte formulas of the viewer frames (include/hybkf.h: kf_render_view / kf_view_model_maps; csrc/view_pixel.h) restated in numpy,
operation for operation in float32, from the float4 maps a raycast wrote and the eye position.  Returns (rows, cols, 4) uint8: b, g, r, a."""
import numpy as np

VIEW_NORMALS, VIEW_SHADED, VIEW_COLOR = 0, 1, 2
f32 = np.float32


def _byte(x):
    """`(unsigned char)x` of a float as the device converts it: truncated towards zero (saturating, NaN -> 0), low byte kept"""
    x = np.asarray(x, np.float32)
    t = np.where(np.isnan(x), f32(0), np.clip(x, f32(-2147483648.0), f32(2147483520.0)))
    return (t.astype(np.int64) & 255).astype(np.uint8)


def view_bytes(mode, v, n, rgb=None, eye=None):
    """v, n: (rows, cols, 4) float32; rgb: (rows, cols, 3) uint8 (COLOR); eye: 3 floats, the pose's translation (SHADED)"""
    v, n = np.asarray(v, np.float32), np.asarray(n, np.float32)
    hit = v[..., 3] == f32(1.0)
    out = np.zeros(v.shape[:2] + (4,), np.uint8)
    out[..., 3] = np.where(hit, 255, 0)
    if mode == VIEW_NORMALS:
        for c in range(3):
            out[..., c] = _byte((f32(255.0) * (n[..., c] + f32(1.0))) / f32(2.0))
    elif mode == VIEW_SHADED:
        e = np.asarray(eye, np.float32).reshape(3)
        with np.errstate(invalid="ignore", divide="ignore"):
            dx, dy, dz = e[0] - v[..., 0], e[1] - v[..., 1], e[2] - v[..., 2]
            s = (dx * dx + dy * dy) + dz * dz
            c = ((n[..., 0] * dx + n[..., 1] * dy) + n[..., 2] * dz) / np.sqrt(s)
            c = np.where(np.isnan(c), f32(0.0), c)                       # fmaxf(NaN, 0) = 0
            c = np.minimum(np.maximum(c, f32(0.0)), f32(1.0))
            g = np.where(hit, _byte(f32(32.0) + f32(223.0) * c), 0).astype(np.uint8)
        assert s.dtype == np.float32 and c.dtype == np.float32
        out[..., 0] = out[..., 1] = out[..., 2] = g
    elif mode == VIEW_COLOR:
        out[..., :3] = np.asarray(rgb, np.uint8)
    else:
        raise ValueError(mode)
    return out
