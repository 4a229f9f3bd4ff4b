"""CPU-only: the ABI of merging maps.  kf_merge_brick_store and kf_refill_window are exported, bound, declared and refuse a NULL context; the host
shim's names and the Python methods exist and answer -1 without an application; the slab shim always answers -1.  The key offset of a merge
(host/map_file.cpp: hkf_map_offset_keys with its overflow-safe range check, hkf_map_info_offset) runs in a stand-alone program with a main of its own
(tests/map_merge_main.cpp), built with AddressSanitizer + UBSan: nothing of it is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kf_merge_brick_store", "kf_refill_window"]


def test_symbols_exported_bound_and_declared():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"^int %s\(kf_ctx\* ctx" % name, header, re.M), name
    assert len(lib.kf_merge_brick_store.argtypes) == 7 and len(lib.kf_refill_window.argtypes) == 1
    for name in ("merge_brick_store", "refill_window"):
        assert hasattr(K.Context, name), name


def test_null_context_is_an_argument_error():
    lib = K.load()
    keys, t, w = np.zeros((1, 3), np.int32), np.zeros(512, np.float32), np.ones(512, np.float32)
    off = (C.c_int32 * 3)(1, 2, 3)
    assert lib.kf_merge_brick_store(None, 1, K._p(keys), K._p(t), K._p(w), None, None) == 1001
    assert lib.kf_merge_brick_store(None, 1, K._p(keys), K._p(t), K._p(w), None, off) == 1001
    assert lib.kf_merge_brick_store(None, 0, None, None, None, None, None) == 1001
    assert lib.kf_refill_window(None) == 1001


def test_shims_without_an_application():
    h = H.load()
    assert hasattr(h, "hkf_app_merge_map") and h.hkf_app_merge_map(b"/nonexistent/x", 0, 0, 0) == -1
    assert h.hkf_app_merge_map(b"/nonexistent/x", 3, -2, 5) == -1
    s = H.load_slabs()                                            # the slab class refuses: the store stays a single-GPU feature
    assert hasattr(s, "hkf_slabs_merge_map") and s.hkf_slabs_merge_map(b"/nonexistent/x", 0, 0, 0) == -1
    assert hasattr(H.App, "merge_map") and hasattr(H.SlabsApp, "merge_map")


def test_offset_helper_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_merge_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "host"), "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"),
                           os.path.join(ROOT, "tests", "map_merge_main.cpp"), os.path.join(ROOT, "hybkinectfu_amd", "host", "map_file.cpp"), "-o", exe])
    work = tmp_path / "maps"
    work.mkdir()
    out = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map merge ok", out.stdout[-3000:]
