"""CPU-only: the ABI of saving and loading the map.  kf_write_brick_store, kf_brick_store_capture and kf_place_window are exported, bound and refuse a
NULL context; the host shim's names exist; map_file_info reads files that numpy writes from the format text of host/map_file.hpp (little-endian:
8 bytes of magic, then the header fields at fixed offsets, 128 bytes in all, then the records sorted by key (z, y, x)) and refuses truncated files, a
wrong magic and keys that are unsorted, doubled or out of range.  The codec itself (host/map_file.cpp) and the duplicate-key check
(csrc/brick_keys_unique.h) run in a stand-alone program with a main of its own (tests/map_file_main.cpp), built with AddressSanitizer + UBSan:
nothing of it is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kf_write_brick_store", "kf_brick_store_capture", "kf_place_window"]
LIM = 1 << 20
ERR_MAGIC, ERR_VERSION, ERR_BRICK, ERR_LENGTH, ERR_KEYS = -2, -3, -4, -5, -6


def test_symbols_exported():
    lib = K.load()
    for name in NEW:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    h = H.load()
    for name in ("hkf_app_save_map", "hkf_app_load_map", "hkf_app_frame_id", "hkf_map_file_info"):
        assert hasattr(h, name), name
    for name in ("save_map", "load_map", "frame_id"):
        assert hasattr(H.App, name), name
    for name in ("write_brick_store", "brick_store_capture", "place_window"):
        assert hasattr(K.Context, name), name


def test_null_context_is_an_argument_error():
    lib = K.load()
    keys, t, w = np.zeros((1, 3), np.int32), np.zeros(512, np.float32), np.ones(512, np.float32)
    assert lib.kf_write_brick_store(None, 1, K._p(keys), K._p(t), K._p(w), None) == 1001
    assert lib.kf_write_brick_store(None, 0, None, None, None, None) == 1001
    assert lib.kf_brick_store_capture(None) == 1001
    assert lib.kf_place_window(None, 0, 0, 0) == 1001
    assert lib.kf_place_window(None, 4, 0, 0) == 1001


def test_shims_without_an_application():
    h = H.load()
    assert h.hkf_app_save_map(b"/nonexistent/x") == -1 and h.hkf_app_load_map(b"/nonexistent/x") == -1 and h.hkf_app_frame_id() == -1
    s = H.load_slabs()                                            # the slab class refuses: the store stays a single-GPU feature
    assert s.hkf_slabs_save_map(b"/nonexistent/x") == -1 and s.hkf_slabs_load_map(b"/nonexistent/x") == -1
    assert hasattr(H.SlabsApp, "save_map") and hasattr(H.SlabsApp, "load_map")


# ---- files written by numpy from the format text ----------------------------------------------------------------------------------------------
def map_bytes(keys, color=False, res=64, size=2.0, max_weight=128.0, origin=(32, -8, 16), frame_id=5, pose=None, dropped=0, magic=b"HYBKFMAP",
              version=1, edge=8, n=None):
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    pose = np.arange(16, dtype=np.float32) * np.float32(0.5) if pose is None else np.asarray(pose, np.float32).reshape(16)
    head = magic + struct.pack("<IIII", version, res, edge, int(color)) + struct.pack("<ff", size, max_weight) + struct.pack("<iii", *origin) + \
        struct.pack("<I", frame_id) + pose.astype("<f4").tobytes() + struct.pack("<QQ", len(keys) if n is None else n, dropped)
    assert len(head) == 128
    rng = np.random.default_rng(7)
    body = b""
    for k in keys:
        body += k.astype("<i4").tobytes() + rng.standard_normal(512).astype("<f4").tobytes() + rng.integers(0, 100, 512).astype("<f4").tobytes()
        if color:
            body += rng.integers(0, 256, 1536).astype(np.uint8).tobytes()
    return head + body


SORTED = [(-3, 2, -1), (0, 0, 0), (1, 0, 0), (-LIM, 1, 0), (5, -4, 2), (LIM - 1, LIM - 1, LIM - 1)]      # ascending by (z, y, x)


def write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@pytest.mark.parametrize("color", [False, True])
def test_info_reads_the_header(tmp_path, color):
    pose = np.linspace(-1, 1, 16, dtype=np.float32)
    info = H.map_file_info(write(tmp_path, "ok.hkfmap", map_bytes(SORTED, color, res=72, size=2.25, max_weight=64.0, origin=(-72, 8, 0), frame_id=9, pose=pose,
                                                                   dropped=4)))
    assert (info["version"], info["resolution"], info["brick_edge"], info["has_color"]) == (1, 72, 8, color)
    assert (info["size"], info["max_weight"], info["origin_vox"], info["frame_id"]) == (2.25, 64.0, (-72, 8, 0), 9)
    assert (info["n_bricks"], info["dropped"]) == (len(SORTED), 4)
    assert np.array_equal(info["pose"].view(np.uint32), pose.reshape(4, 4).view(np.uint32))
    assert H.map_file_info(write(tmp_path, "empty.hkfmap", map_bytes([], color)))["n_bricks"] == 0


def refused(path):
    h = H.load()
    h.hkf_map_file_info.argtypes = [H.C.c_char_p] + [H.C.c_void_p] * 6
    return h.hkf_map_file_info(os.fsencode(path), None, None, None, None, None, None)


def test_info_refuses_what_the_reader_refuses(tmp_path):
    good = map_bytes(SORTED, True)
    assert refused(write(tmp_path, "good", good)) == 0
    assert refused(write(tmp_path, "short", good[:-1])) == ERR_LENGTH
    assert refused(write(tmp_path, "long", good + b"\0")) == ERR_LENGTH
    assert refused(write(tmp_path, "head", good[:127])) == ERR_MAGIC
    assert refused(write(tmp_path, "none", b"")) == ERR_MAGIC
    assert refused(write(tmp_path, "count", map_bytes(SORTED, n=len(SORTED) + 1))) == ERR_LENGTH
    assert refused(write(tmp_path, "flag", map_bytes(SORTED, False)[:20] + struct.pack("<I", 1) + map_bytes(SORTED, False)[24:])) == ERR_LENGTH   # colour flag set, records without
    assert refused(write(tmp_path, "magic", map_bytes(SORTED, magic=b"HYBKFMAQ"))) == ERR_MAGIC
    assert refused(write(tmp_path, "version", map_bytes(SORTED, version=2))) == ERR_VERSION
    assert refused(write(tmp_path, "edge", map_bytes(SORTED, edge=16))) == ERR_BRICK
    unsorted = [SORTED[1], SORTED[0]] + SORTED[2:]
    assert refused(write(tmp_path, "unsorted", map_bytes(unsorted))) == ERR_KEYS
    assert refused(write(tmp_path, "x_before_y", map_bytes([(0, 1, 0), (1, 0, 0)]))) == ERR_KEYS      # (1, 0, 0) sorts first: y outranks x
    assert refused(write(tmp_path, "twice", map_bytes(SORTED[:2] + SORTED[1:]))) == ERR_KEYS
    for bad in ((LIM, 0, 0), (0, -LIM - 1, 0), (0, 0, 1 << 21)):
        assert refused(write(tmp_path, "range", map_bytes([bad]))) == ERR_KEYS, bad
    assert refused(str(tmp_path / "missing")) == -1
    with pytest.raises(K.KfError):
        H.map_file_info(write(tmp_path, "short2", good[:-1]))


# ---- the codec and the duplicate-key check under sanitizers, in a process of their own ------------------------------------------------------------
def test_codec_round_trip_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_file_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "host"), "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"),
                           os.path.join(ROOT, "tests", "map_file_main.cpp"), os.path.join(ROOT, "hybkinectfu_amd", "host", "map_file.cpp"), "-o", exe])
    work = tmp_path / "maps"
    work.mkdir()
    out = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map file ok", out.stdout[-3000:]
