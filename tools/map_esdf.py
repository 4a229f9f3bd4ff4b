#!/usr/bin/env python3
"""The distance field of a map file over a box, on the device (kf_map_distance_field): for every voxel of the box the distance in metres to the nearest
obstacle voxel of the map (tsdf <= level; with --unknown-is-obstacle also every voxel nobody observed), up to --radius metres, and the class bytes.  The box
is in WORLD metres -- the first cube's coordinates, those of the map mesh's vertices --, half-open: a voxel is in it iff its centre (g + 1/2) * cell is
(tools/map_crop.py's rule); --bounds takes the box of the map's bricks instead.  The radius is floor(M / cell) voxels, clamped to 1 .. 255.  A box with an
edge above 128 voxels is computed in tiles and stitched, which is exact.  OUT.npz holds dist (nz, ny, nx) float32, inf where no obstacle lies within the
radius, cls (nz, ny, nx) uint8 (0 unknown, 1 free, 2 occupied), lo_vox (x, y, z) and cell.
usage: tools/map_esdf.py IN.map OUT.npz [--box x0 y0 z0 x1 y1 z1 | --bounds] [--radius M] [--level L] [--unknown-is-obstacle]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from hybkinectfu_amd import host_app as H, lib as K
import map_crop

TILE = 128


def field(ctx, lo, dims, radius, level, site_mask):
    """(dist2, cls) of the box, in tiles of at most TILE voxels per axis (the field of a box is the same bytes as that part of the field of any box around it)"""
    nx, ny, nz = dims
    d2, cls = np.zeros((nz, ny, nx), np.uint16), np.zeros((nz, ny, nx), np.uint8)
    for z in range(0, nz, TILE):
        for y in range(0, ny, TILE):
            for x in range(0, nx, TILE):
                n = (min(TILE, nx - x), min(TILE, ny - y), min(TILE, nz - z))
                out = ctx.map_distance_field((lo[0] + x, lo[1] + y, lo[2] + z), n, radius, level, site_mask)
                d2[z:z + n[2], y:y + n[1], x:x + n[0]] = out["dist2"]
                cls[z:z + n[2], y:y + n[1], x:x + n[0]] = out["cls"]
    return d2, cls


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", metavar="IN.map")
    ap.add_argument("dst", metavar="OUT.npz")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--box", type=float, nargs=6, metavar=("x0", "y0", "z0", "x1", "y1", "z1"))
    g.add_argument("--bounds", action="store_true", help="the box of the map's bricks (the default)")
    ap.add_argument("--radius", type=float, default=1.0, metavar="M", help="the greatest distance reported, metres")
    ap.add_argument("--level", type=float, default=0.0, help="a voxel is an obstacle where tsdf <= level")
    ap.add_argument("--unknown-is-obstacle", action="store_true")
    a = ap.parse_args(argv)
    if (a.box and any(v != v for v in a.box)) or a.radius != a.radius or a.level != a.level:
        print("map_esdf: a NaN argument", file=sys.stderr)
        return 2
    info = H.map_file_info(a.src)                                 # every check of the reader; raises for a file it refuses
    res, color, size = info["resolution"], info["has_color"], info["size"]
    m = map_crop.read_records(open(a.src, "rb").read(), color)
    cell = np.float32(size) / np.float32(res)                     # the fp32 quotient the volume uses
    radius = int(min(255, max(1, np.floor(np.float64(np.float32(a.radius)) / np.float64(cell)))))
    cam = K.camera(160, 120, 79.5, 59.5, 131.25, 131.25)         # (a context needs a camera; no image is ever processed)
    ctx = K.Context(cam, res, size, info["max_weight"], has_color=color)
    try:
        ctx.brick_store_reserve(max(1, len(m[0])))
        ctx.place_window(0, 0, -(1 << 22))                        # the window stands far from any map: the store alone is the map
        if len(m[0]):
            ctx.write_brick_store(m[0], m[1], m[2], m[3])
        if a.box:
            lo, hi = map_crop.box_voxels(a.box[:3], a.box[3:], cell)
        else:
            blo, bhi = ctx.brick_store_bounds()
            lo, hi = tuple(8 * v for v in blo), tuple(8 * v for v in bhi)
        dims = tuple(h - l for l, h in zip(lo, hi))
        if any(n <= 0 for n in dims):
            print("map_esdf: an empty box", file=sys.stderr)
            return 2
        mask = (1 << K.VOX_OCCUPIED) | ((1 << K.VOX_UNKNOWN) if a.unknown_is_obstacle else 0)
        d2, cls = field(ctx, lo, dims, radius, a.level, mask)
    finally:
        ctx.close()
    dist = np.where(d2 == K.EDT_FAR, np.float32(np.inf), np.sqrt(d2.astype(np.float32)) * cell).astype(np.float32)
    np.savez_compressed(a.dst, dist=dist, cls=cls, lo_vox=np.array(lo, np.int32), cell=cell)
    print("map_esdf: %s: %d bricks; voxels %s + %s, radius %d voxels: %d of %d voxels within it -> %s" % (
        a.src, len(m[0]), lo, dims, radius, int(np.count_nonzero(d2 != K.EDT_FAR)), d2.size, a.dst))
    return 0


if __name__ == "__main__":
    sys.exit(main())
