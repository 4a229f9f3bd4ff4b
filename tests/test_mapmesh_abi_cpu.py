"""CPU-only: the map mesh's ABI (kf_marching_cubes_at, kf_brick_store_bounds, kf_marching_cubes_map, kf_map_tile_frames and the host shim's
hkf_app_set_map_mesh) is exported, bound and refuses NULL; and the tile lattice of kf_marching_cubes_map -- csrc/map_tiles.h -- is checked against a
brute-force numpy statement of it: every world cell inside the bounds is owned by exactly one visited tile, every visited frame meets the bounds, all
frames are multiples of 8, the order is z, y, x ascending.  The header is also compiled into a stand-alone program with a main of its own, built with
AddressSanitizer + UBSan and run on the CPU over the same cases: nothing is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kf_marching_cubes_at", "kf_brick_store_bounds", "kf_marching_cubes_map", "kf_map_tile_frames"]

# (res, store lo, store hi (bricks, half-open; lo == hi: no store), window origin (voxels))
CASES = [
    (32, (0, 0, 0), (0, 0, 0), (0, 0, 0)),
    (32, (-3, -1, 0), (2, 1, 5), (-8, 16, 40)),
    (64, (0, 0, 0), (0, 0, 0), (0, 0, 0)),
    (64, (0, 0, 0), (0, 0, 0), (32, 32, 0)),
    (64, (1, 1, 1), (7, 7, 7), (32, 0, 0)),
    (64, (-9, -2, 3), (-1, 6, 12), (-40, 8, 24)),
    (64, (-20, -20, -20), (-14, -15, -16), (96, 48, 0)),       # store and window far apart: nothing in between is visited
    (72, (0, 0, 0), (0, 0, 0), (-24, 24, -16)),
    (72, (-5, 0, -7), (9, 9, 2), (0, 0, -16)),
    (72, (6, 6, 6), (7, 7, 7), (56, 56, 56)),                  # one brick, exactly at a lattice line (T = 56)
]


def test_symbols_exported_and_bound():
    lib = K.load()
    for name in NEW:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    for name in ("marching_cubes_at", "brick_store_bounds", "marching_cubes_map"):
        assert callable(getattr(K.Context, name)), name
    h = H.load()
    assert hasattr(h, "hkf_app_set_map_mesh") and callable(H.App.set_map_mesh)
    slabs = C.CDLL(os.path.join(ROOT, "hybkinectfu_amd", "libhybkf_slabs.so"))      # links the host library and libhybkf.so: the new names resolve through it too
    assert hasattr(slabs, "hkf_slabs_generate_mesh")


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(K.SYMBOLS) and set(NEW) <= declared


def test_null_is_an_argument_error():
    lib = K.load()
    z = (C.c_int32 * 3)(0, 0, 0)
    assert lib.kf_marching_cubes_at(None, 0, 0.1, z, z, z, 0) == 1001
    assert lib.kf_brick_store_bounds(None, z, z) == 1001
    n = C.c_uint32(7)
    assert lib.kf_marching_cubes_map(None, 0, 0.1, 1, C.byref(n)) == 1001 and n.value == 0
    assert lib.kf_map_tile_frames(None, z, z, 64, None, 0) == -1
    assert lib.kf_map_tile_frames(z, z, z, 24, None, 0) == -1           # below 32
    assert lib.kf_map_tile_frames(z, z, z, 68, None, 0) == -1           # no multiple of 8


def boxes_of(res, slo, shi, origin):
    """the voxel boxes the map covers: the window, and the store's bounds when it holds something"""
    b = [(np.array(origin, np.int64), np.array(origin, np.int64) + res)]
    if all(l < h for l, h in zip(slo, shi)):
        b.append((np.array(slo, np.int64) * 8, np.array(shi, np.int64) * 8))
    return b


def check_lattice(res, slo, shi, origin, frames):
    T = res - 16
    frames = np.asarray(frames, np.int64).reshape(-1, 3)
    assert np.all(frames % 8 == 0)
    assert np.all((frames + 8) % T == 0)                          # F_k = k T - 8
    key = [tuple(f[::-1]) for f in frames.tolist()]
    assert key == sorted(key) and len(set(key)) == len(key)       # z, then y, then x, ascending, no tile twice
    bxs = boxes_of(res, slo, shi, origin)
    for f in frames:                                              # nothing visited in vain: the frame meets the window or the store's box
        assert any(np.all(f < hi) and np.all(f + res > lo) for lo, hi in bxs), f
    # brute force: every world cell of every box is owned by exactly one visited tile (tile F owns the world cells [F + 8, F + res - 8))
    for lo, hi in bxs:
        z, y, x = np.meshgrid(*[np.arange(lo[k], hi[k]) for k in (2, 1, 0)], indexing="ij")
        owners = np.zeros(z.shape, np.int32)
        for f in frames:
            owners += ((x >= f[0] + 8) & (x < f[0] + res - 8) & (y >= f[1] + 8) & (y < f[1] + res - 8) & (z >= f[2] + 8) & (z < f[2] + res - 8))
        assert np.all(owners == 1), (res, slo, shi, origin)
    # ... and the brute-force statement of "visited": a lattice tile in a generous range is visited exactly when its frame meets a box
    want = set()
    for lo, hi in bxs:
        k0, k1 = (lo - res) // T - 1, hi // T + 2
        for kz in range(k0[2], k1[2]):
            for ky in range(k0[1], k1[1]):
                for kx in range(k0[0], k1[0]):
                    f = np.array([kx, ky, kz]) * T - 8
                    if np.all(f < hi) and np.all(f + res > lo):
                        want.add(tuple(f.tolist()))
    assert want == {tuple(f) for f in frames.tolist()}


@pytest.mark.parametrize("case", CASES)
def test_lattice_against_brute_force(case):
    res, slo, shi, origin = case
    frames = K.map_tiles(slo, shi, origin, res)
    assert len(frames) >= 1
    check_lattice(res, slo, shi, origin, frames)


@pytest.fixture(scope="module")
def tiles_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_tiles") / "map_tiles_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "map_tiles_main.cpp"), "-o", exe])
    return exe


def test_lattice_program_under_sanitizers(tiles_program):
    text = "".join("%d %d %d %d %d %d %d %d %d %d\n" % ((c[0],) + tuple(c[1]) + tuple(c[2]) + tuple(c[3])) for c in CASES) + "24 0 0 0 0 0 0 0 0 0\n"
    out = subprocess.run([tiles_program], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "map tiles ok %d" % (len(CASES) + 1), out.stdout[-2000:]
    at = 0
    for res, slo, shi, origin in CASES:
        n = int(lines[at].split()[1])
        frames = np.array([[int(v) for v in l.split()] for l in lines[at + 1:at + 1 + n]], np.int64).reshape(-1, 3)
        at += 1 + n
        assert np.array_equal(frames, K.map_tiles(slo, shi, origin, res))          # the program and the library say the same
        check_lattice(res, slo, shi, origin, frames)
    assert lines[at] == "tiles -1"                                # res 24: refused
