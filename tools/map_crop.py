#!/usr/bin/env python3
"""A map file with a box erased from it, or cropped to the box, on the device (kf_brick_store_erase_box), and optionally without its weakly observed bricks
(kf_brick_store_erase_weak).  The box is in WORLD metres -- the first cube's coordinates, those of the map mesh's vertices --, half-open: a voxel goes iff
its centre (g + 1/2) * cell lies in it (with --outside: iff it does not, which crops the map to the box).  The header keeps everything but the brick count;
the records are sorted by key (z, y, x).
usage: tools/map_crop.py IN OUT --box x0 y0 z0 x1 y1 z1 [--outside] [--min-weight W]"""
import argparse
import ctypes as C
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from hybkinectfu_amd import host_app as H, lib as K

RECORD = {False: 12 + 4096, True: 12 + 4096 + 1536}


def read_records(data, color):
    rec = RECORD[color]
    n = (len(data) - 128) // rec
    raw = np.frombuffer(data, np.uint8, offset=128).reshape(n, rec)
    keys = np.ascontiguousarray(raw[:, :12]).view("<i4").reshape(n, 3)
    t = np.ascontiguousarray(raw[:, 12:2060]).view("<f4").reshape(n, 8, 8, 8)
    w = np.ascontiguousarray(raw[:, 2060:4108]).view("<f4").reshape(n, 8, 8, 8)
    c = np.ascontiguousarray(raw[:, 4108:]).reshape(n, 8, 8, 8, 3) if color else None
    return keys, t, w, c


def record_bytes(m):
    n = len(m[0])
    if n == 0:
        return b""
    parts = [np.ascontiguousarray(m[0], "<i4").reshape(n, -1).view(np.uint8), np.ascontiguousarray(m[1], "<f4").reshape(n, -1).view(np.uint8),
             np.ascontiguousarray(m[2], "<f4").reshape(n, -1).view(np.uint8)] + ([m[3].reshape(n, -1)] if m[3] is not None else [])
    return np.concatenate(parts, axis=1).tobytes()


def box_voxels(lo_m, hi_m, cell):
    """hkf_erase_map_box_voxels: ceil(x / cell - 1/2) at both ends, clamped to the key range"""
    lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    l, h = (C.c_float * 3)(*[float(v) for v in lo_m]), (C.c_float * 3)(*[float(v) for v in hi_m])
    if H.load().hkf_erase_map_box_voxels(l, h, C.c_float(cell), lo, hi) != 0:
        raise K.KfError("hkf_erase_map_box_voxels failed")
    return tuple(lo), tuple(hi)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", metavar="IN")
    ap.add_argument("dst", metavar="OUT")
    ap.add_argument("--box", type=float, nargs=6, required=True, metavar=("x0", "y0", "z0", "x1", "y1", "z1"))
    ap.add_argument("--outside", action="store_true", help="clear what lies outside the box: crop the map to it")
    ap.add_argument("--min-weight", type=float, default=0.0, help="afterwards, remove every brick whose greatest weight is below this")
    a = ap.parse_args(argv)
    if any(v != v for v in a.box) or a.min_weight != a.min_weight:
        print("map_crop: a NaN argument", file=sys.stderr)
        return 2
    info = H.map_file_info(a.src)                                 # every check of the reader; raises for a file it refuses
    res, color, size = info["resolution"], info["has_color"], info["size"]
    data = open(a.src, "rb").read()
    m = read_records(data, color)
    cell = np.float32(size) / np.float32(res)                     # the fp32 quotient the volume uses
    lo, hi = box_voxels(a.box[:3], a.box[3:], cell)
    cam = K.camera(160, 120, 79.5, 59.5, 131.25, 131.25)         # (a context needs a camera; no image is ever processed)
    ctx = K.Context(cam, res, size, info["max_weight"], has_color=color)
    try:
        ctx.brick_store_reserve(max(1, len(m[0])))
        if len(m[0]):
            ctx.write_brick_store(m[0], m[1], m[2], m[3])
        removed, cleared = ctx.brick_store_erase_box(lo, hi, K.ERASE_OUTSIDE if a.outside else K.ERASE_INSIDE)
        weak = ctx.brick_store_erase_weak(a.min_weight) if a.min_weight > 0 else 0
        keys, t, w, c = ctx.brick_store(color=color)
        o = np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))
        m = (keys[o], t[o], w[o], c[o] if color else None)
    finally:
        ctx.close()
    head = bytearray(data[:128])
    struct.pack_into("<Q", head, 112, len(m[0]))
    with open(a.dst, "wb") as f:
        f.write(bytes(head) + record_bytes(m))
    print("map_crop: %s: %d bricks -> %s: %d bricks; voxels %s - %s %s: %d bricks removed, %d observed voxels cleared; %d weak bricks removed" % (
        a.src, info["n_bricks"], a.dst, len(m[0]), lo, hi, "kept" if a.outside else "erased", removed, cleared, weak))
    return 0


if __name__ == "__main__":
    sys.exit(main())
