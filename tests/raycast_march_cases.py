"""The cases of tests/test_gpu_raycast_march.py, shared by the parent (oracle) and its child process (GPU): the smallest volumes at which each path of
the instantiated march trip and of the tile prologue first exists.  Volumes and viewpoints are raycast_scenarios.py's, by import."""
import numpy as np

import raycast_scenarios as R

# id -> (volume id, res, size, camera, view names)
CASES = {
    # the size is a power of two, the resolution is not: two multiplications per axis, general table indices (12 bricks, 3 macro, 6 meso cells per axis)
    "m96": ("m96", 96, 4.0, R.RAGGED, ("graze-y", "inside-diag", "corner-mixed", "axes-x", "macro-plane")),
    # both powers of two, but res < size: the scaling is DOWN (1/2) and the one-multiplication form must not be taken; near / far scaled like the volume
    "m64": ("m64", 64, 128.0, R.RAGGED, ("front+z", "inside-diag")),
    # 256^3 @ 4 m: the meso scan with 16 cells (two bytes) per row -- or, KF_RAYCAST_BOUNDS_MESO=0, the macro scan with 8 cells, one byte, per row
    "m256": ("m256", 256, 4.0, R.RAGGED, ("graze-y", "far", "corner-low", "inside+z", "near-far-cut", "away")),
    # 128^3 @ 4 m under KF_RAYCAST_NEG_LDS=0 / KF_RAYCAST_MESO=0: the conditional flag read and the absent meso lookup
    "m128": ("m128", 128, 4.0, R.RAGGED, ("graze-y",)),
}
# the same 128^3 volume in two z-slabs: the second one stores layers [48, 128) and owns [64, 128)
SLAB_CASE = ("m128", 128, 4.0, R.RAGGED, ("graze-y", "inside-diag"))
SLAB_RANGES = ((0, 64), (64, 128))
SLAB_HALO = 16
VOLUME_IDS = ("m96", "m64", "m256", "m128")


def key(k):
    return k.replace("/", "__")


def calls(case):
    """[(key, view name, pose float32, near, far)] of a case, in the order both sides cast them"""
    vid, res, size, cam, names = case
    # (raycast_scenarios' near / far planes are metres at its 3-4 m volumes: a 128 m volume scales them)
    scale = size / 4.0 if size > 8.0 else 1.0
    out = []
    for name, pose, near, far in R.views(size, res):
        if name in names:
            out.append(("%s/%s" % (vid, name), name, pose.astype(np.float32), near * scale, far * scale))
    assert len(out) == len(names)
    return out


def as_scenario(case):
    """the case as raycast_scenarios describes a volume (for oracle_volume / oracle_maps) and its calls in that module's shape"""
    vid, res, size, cam, names = case
    vol = (vid, res, size, False, [(cam, names)])
    return vol, [(k, cam, name, pose, near, far) for k, name, pose, near, far in calls(case)]
