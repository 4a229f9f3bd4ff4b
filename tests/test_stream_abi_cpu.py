"""CPU-only: the ABI of the streamed mesh -- region extraction, world soup, stream-out -- is declared, bound and exported and refuses NULL
arguments; hkf_departing_boxes (which cells a shift makes unextractable for good) agrees with a brute-force numpy statement of the rule over all
sign patterns; and the same code passes a stand-alone AddressSanitizer + UBSan run."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kf_marching_cubes_region", "kf_region_work", "kf_world_soup_reserve", "kf_world_soup_count", "kf_read_world_soup", "kf_clear_world_soup",
       "kf_append_world_soup", "kf_set_stream_out"]
ARG = 1001


def test_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hybkf.h")).read(), flags=re.S)
    lib = K.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in K.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"KF_MC_WORLD\s*=\s*1\b", header) and re.search(r"KF_MC_TO_WORLD_SOUP\s*=\s*2\b", header)
    assert (K.MC_WORLD, K.MC_TO_WORLD_SOUP) == (1, 2)
    for method in ("marching_cubes_region", "region_work", "world_soup_reserve", "world_soup_count", "world_soup", "clear_world_soup",
                   "append_world_soup", "set_stream_out"):
        assert callable(getattr(K.Context, method)), method
    h = H.load()
    for name in ("hkf_departing_boxes", "hkf_app_set_stream_mesh", "hkf_app_world_soup_count"):
        assert hasattr(h, name), name
    assert callable(H.App.set_stream_mesh) and callable(H.App.world_soup_count)


def test_null_arguments_are_argument_errors():
    lib = K.load()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    n, d = C.c_uint32(), C.c_uint32()
    tri = np.zeros(1, K.TRI_DTYPE)
    assert lib.kf_marching_cubes_region(None, 0, 1.0, lo, hi, 0) == ARG
    assert lib.kf_region_work(None, (C.c_uint64 * 2)()) == ARG
    assert lib.kf_world_soup_reserve(None, 10) == ARG
    assert lib.kf_world_soup_count(None, C.byref(n), C.byref(d)) == ARG
    assert lib.kf_read_world_soup(None, tri.ctypes.data_as(C.c_void_p), 0, 1) == ARG
    assert lib.kf_clear_world_soup(None) == ARG
    assert lib.kf_append_world_soup(None) == ARG
    assert lib.kf_set_stream_out(None, 1, 0, 1.0) == ARG
    assert lib.kf_set_stream_out(None, 0, 0, 1.0) == ARG
    assert H.load().hkf_app_set_stream_mesh(100) == -1 and H.load().hkf_app_world_soup_count() == -1      # no application


def brute_force(d, R):
    """mark every cell whose 27-voxel stencil (x-1 .. x+1 each way, inside the volume) meets a voxel that leaves when the window moves by d"""
    axes = []
    for k in range(3):
        v = np.arange(R)
        leaves = (v < d[k]) if d[k] > 0 else ((v >= R + d[k]) if d[k] < 0 else np.zeros(R, bool))
        cell = leaves.copy()
        cell[1:] |= leaves[:-1]
        cell[:-1] |= leaves[1:]
        axes.append(cell)
    return axes[2][:, None, None] | axes[1][None, :, None] | axes[0][None, None, :]           # (z, y, x)


@pytest.mark.parametrize("R", [64, 72])
def test_departing_boxes_match_the_rule(R):
    mags = (8, 24)
    cases = set()
    for signs in itertools.product((-1, 0, 1), repeat=3):            # all 27 sign patterns
        for m in itertools.product(mags, repeat=3):
            cases.add(tuple(s * v for s, v in zip(signs, m)))
    cases |= {(R, 0, 0), (0, -R, 8), (R + 8, -R - 8, R), (-8, 0, R - 8), (R - 8, 8 - R, 0)}
    for d in sorted(cases):
        boxes = H.departing_boxes(d, R)
        hits = np.zeros((R, R, R), np.int32)
        for lo, hi in boxes:
            assert all(0 <= a < b <= R for a, b in zip(lo, hi)), (d, lo, hi)
            hits[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] += 1
        assert hits.max(initial=0) <= 1, d                           # disjoint
        assert np.array_equal(hits == 1, brute_force(d, R)), d       # and exactly the cells of the rule
        assert len(boxes) <= sum(1 for x in d if x)
    assert H.departing_boxes((8, 0, 0), R) == [((0, 0, 0), (9, R, R))]
    assert H.departing_boxes((-8, 0, 0), R) == [((R - 9, 0, 0), (R, R, R))]
    assert H.departing_boxes((16, -8, 24), R) == [((0, 0, 0), (17, R, R)), ((17, R - 9, 0), (R, R, R)), ((17, 0, 0), (R, R - 9, 25))]
    assert H.departing_boxes((0, 0, 0), R) == []


def test_departing_boxes_under_sanitizers(tmp_path):
    """recentre.cpp + a main of its own, -fsanitize=address,undefined, run on the CPU: nothing is loaded into Python"""
    host = os.path.join(ROOT, "hybkinectfu_amd", "host")
    exe = str(tmp_path / "stream_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fsanitize=float-cast-overflow", "-ffp-contract=off", "-I", host, os.path.join(ROOT, "tests", "stream_host_main.cpp"),
                           os.path.join(host, "recentre.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "stream host arithmetic ok" in out.stdout, out.stdout


def test_strip_boxes_under_sanitizers(tmp_path):
    """strip_boxes.h (the one statement of the strip rule, behind hkf_departing_boxes, the stream-out's boxes and the brick store's) + a main of its
    own, -fsanitize=address,undefined, run on the CPU: n in {1, 2, 5, 8}, both reaches, every move in [-n-2, n+2]^3; nothing is loaded into Python"""
    exe = str(tmp_path / "strip_boxes_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "strip_boxes_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "strip boxes ok" in out.stdout, out.stdout
