#!/usr/bin/env python3
"""A coarser copy of a map file: the map halved L times on the device (kf_merge_brick_store_halved: the mean tsdf of the observed children, their least
weight, their mean colour), written as a map file of resolution / 2^L that loadMap takes in an application of that resolution.  The header keeps size, max
weight, colour flag, frame id and dropped count; origin_vox becomes 8 * floor(origin / 2^L / 8) per axis and the pose's translation moves by
origin * s - origin_new * s_new metres (float64, rounded to float32 once), as HybKinectfu::loadMapCoarser places them; the records are sorted by key (z, y, x).
usage: tools/map_lod.py IN OUT [--levels L]      (L in 1..3, default 1; resolution / 2^L must be a multiple of 8)"""
import argparse
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
    parts = [np.ascontiguousarray(m[0], "<i4").reshape(n, -1).view(np.uint8), np.ascontiguousarray(m[1], "<f4").reshape(n, -1).view(np.uint8),
             np.ascontiguousarray(m[2], "<f4").reshape(n, -1).view(np.uint8)] + ([m[3].reshape(n, -1)] if m[3] is not None else [])
    return np.concatenate(parts, axis=1).tobytes()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", metavar="IN")
    ap.add_argument("dst", metavar="OUT")
    ap.add_argument("--levels", type=int, default=1)
    a = ap.parse_args(argv)
    info = H.map_file_info(a.src)                                 # every check of the reader; raises for a file it refuses
    res, color, size, levels = info["resolution"], info["has_color"], info["size"], a.levels
    if not 1 <= levels <= 3 or res % (8 << levels):
        print("map_lod: resolution %d cannot be halved %d times into a multiple of 8" % (res, levels), file=sys.stderr)
        return 2
    data = open(a.src, "rb").read()
    m = read_records(data, color)
    new_res = res >> levels
    cam = K.camera(160, 120, 79.5, 59.5, 131.25, 131.25)         # (a context needs a camera; no image is ever processed)
    ctx = K.Context(cam, new_res, size, info["max_weight"], has_color=color)
    try:
        for _ in range(levels):
            ctx.brick_store_reserve(max(1, len(K.halved_brick_keys(m[0]))))          # (reserving clears)
            ctx.merge_brick_store_halved(m[0], m[1], m[2], m[3])
            keys, t, w, c = ctx.brick_store(color=color)
            o = np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))
            m = (keys[o], t[o], w[o], c[o] if color else None)
    finally:
        ctx.close()
    origin = info["origin_vox"]
    new_origin = tuple(8 * (o // (8 << levels)) for o in origin)  # (floor division)
    s, s_new = np.float64(np.float32(size)) / np.float64(res), np.float64(np.float32(size)) / np.float64(new_res)
    pose = info["pose"].astype(np.float32)
    for k in range(3):
        pose[k, 3] = np.float32((np.float64(pose[k, 3]) + np.float64(origin[k]) * s) - np.float64(new_origin[k]) * s_new)
    head = bytearray(data[:128])
    struct.pack_into("<I", head, 12, new_res)
    struct.pack_into("<3i", head, 32, *new_origin)
    head[48:112] = pose.astype("<f4").tobytes()
    struct.pack_into("<Q", head, 112, len(m[0]))
    with open(a.dst, "wb") as f:
        f.write(bytes(head) + record_bytes(m))
    print("map_lod: %s: %d^3, %d bricks -> %s: %d^3, %d bricks, origin %s" % (a.src, res, info["n_bricks"], a.dst, new_res, len(m[0]), (new_origin,)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
