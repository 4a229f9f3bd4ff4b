"""CPU-only: the brick store's ABI (kf_brick_store_reserve, kf_brick_store_count, kf_brick_store_clear, kf_read_brick_store and the host shim's two
names) is exported and refuses a NULL context; header and binding agree; and the key of a brick -- its world brick coordinate packed into 64 bits,
csrc/brick_key.h -- round-trips against a numpy restatement.  The header is compiled into a stand-alone program with a main of its own, built with
AddressSanitizer + UBSan and run on the CPU: nothing is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kf_brick_store_reserve", "kf_brick_store_count", "kf_brick_store_clear", "kf_read_brick_store"]
EMPTY = 0xFFFFFFFFFFFFFFFF                                      # KF_BRICK_KEY_EMPTY: a free entry of the hash table
LIM = 1 << 20


def test_symbols_exported():
    lib = K.load()
    for name in NEW:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    h = H.load()
    for name in ("hkf_app_set_brick_store", "hkf_app_brick_store_count"):
        assert hasattr(h, name), name


def test_header_and_binding_agree():
    txt = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(K.SYMBOLS) and set(NEW) <= declared


def test_null_context_is_an_argument_error():
    lib = K.load()
    assert lib.kf_brick_store_reserve(None, 16) == 1001
    assert lib.kf_brick_store_reserve(None, 0) == 1001
    held, dropped, restored = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert lib.kf_brick_store_count(None, C.byref(held), C.byref(dropped), C.byref(restored)) == 1001
    assert lib.kf_brick_store_count(None, None, None, None) == 1001
    assert lib.kf_brick_store_clear(None) == 1001
    assert lib.kf_read_brick_store(None, 0, 0, None, None, None, None) == 1001


def np_pack(xyz):
    """the key in numpy: three signed 21-bit fields, x lowest"""
    f = (np.asarray(xyz, np.int64) & ((1 << 21) - 1)).astype(np.uint64)
    return f[:, 0] | (f[:, 1] << np.uint64(21)) | (f[:, 2] << np.uint64(42))


def np_unpack(keys):
    out = np.stack([(keys >> np.uint64(21 * k)) & np.uint64((1 << 21) - 1) for k in range(3)], axis=1).astype(np.int64)
    return np.where(out >= LIM, out - (1 << 21), out)


@pytest.fixture(scope="module")
def key_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("brick_key") / "brick_key_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "brick_key_main.cpp"), "-o", exe])
    return exe


def triples():
    corners = [-LIM, -(LIM - 1), 0, LIM - 1]
    t = [(x, y, z) for x in corners for y in corners for z in corners]          # every corner, zero among them
    t += [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (-1, -1, -1)]
    rng = np.random.default_rng(20)
    t += [tuple(int(v) for v in r) for r in rng.integers(-LIM, LIM, size=(1000, 3))]
    return np.array(t, np.int64)


def test_key_round_trip_under_sanitizers(key_program):
    t = triples()
    out = subprocess.run([key_program], input="".join("%d %d %d\n" % tuple(r) for r in t), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "brick keys ok %d" % len(t), out.stdout[-2000:]
    assert int(lines[0], 16) == EMPTY
    rows = [l.split() for l in lines[1:-1]]
    keys = np.array([int(r[0], 16) for r in rows], np.uint64)
    back = np.array([[int(v) for v in r[1:4]] for r in rows], np.int64)
    place = np.array([int(r[4]) for r in rows])
    assert np.array_equal(keys, np_pack(t))                       # pack
    assert np.array_equal(back, t) and np.array_equal(np_unpack(keys), t)       # unpack, both ways round
    assert not np.any(keys == np.uint64(EMPTY)) and not np.any(keys >> np.uint64(63))   # bit 63 is never set: no key is the empty marker
    assert len(set(keys.tolist())) == len(set(map(tuple, t.tolist())))          # distinct coordinates, distinct keys
    assert place.min() >= 0 and place.max() < 2048


def test_out_of_range_coordinate_is_refused(key_program):
    for bad in ("%d 0 0\n" % LIM, "0 %d 0\n" % (-LIM - 1), "0 0 %d\n" % (1 << 21)):
        out = subprocess.run([key_program], input=bad, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 2 and "out of range" in out.stdout, out.stdout
