"""CPU-only: the ABI and the host side of halving a map's resolution.  kf_merge_brick_store_halved and kf_halved_brick_keys are exported, bound, declared
and refuse what they must without a device; the host shim's name and the Python methods exist and answer -1 without an application; the slab shim always
answers -1.  kf_halved_brick_keys is compared with numpy (key >> 1, the arithmetic shift, unique, sorted by (z, y, x)) on random keys that straddle 0 and touch
both ends of the key range."""
import ctypes as C
import os
import re

import numpy as np

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = -(1 << 20), (1 << 20) - 1
ARG = 1001


def np_halved(keys):
    k = np.unique(np.asarray(keys, np.int64).reshape(-1, 3) >> 1, axis=0)
    return k[np.lexsort((k[:, 0], k[:, 1], k[:, 2]))].astype(np.int32)


def raw(keys, out, cap):
    lib = K.load()
    n = 0 if keys is None else len(keys)
    return lib.kf_halved_brick_keys(n, K._p(keys) if keys is not None else None, K._p(out) if out is not None else None, cap)


def random_keys():
    rng = np.random.default_rng(23)
    near = rng.integers(-9, 10, (300, 3))                          # straddling 0, many collisions after the shift
    ends = np.array([[LO, LO, LO], [HI, HI, HI], [LO, HI, 0], [HI - 1, LO + 1, -1], [-1, -1, -1], [-3, -2, 1], [0, 0, 0], [LO + 1, LO, LO]])
    far = rng.integers(LO, HI + 1, (50, 3))
    return np.ascontiguousarray(np.unique(np.concatenate([near, ends, far]), axis=0).astype(np.int32))


def test_symbols_header_and_binding():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name in ("kf_merge_brick_store_halved", "kf_halved_brick_keys"):
        assert hasattr(lib, name) and name in K.SYMBOLS
    assert re.search(r"^int kf_merge_brick_store_halved\(kf_ctx\* ctx, uint32_t count", header, re.M)
    assert re.search(r"^int64_t kf_halved_brick_keys\(uint32_t count", header, re.M)
    assert len(lib.kf_merge_brick_store_halved.argtypes) == 6
    assert len(lib.kf_halved_brick_keys.argtypes) == 4 and lib.kf_halved_brick_keys.restype is C.c_int64
    h = H.load()
    assert hasattr(h, "hkf_app_load_map_coarser") and h.hkf_app_load_map_coarser(b"/nonexistent/x") == -1     # no application
    s = H.load_slabs()
    assert hasattr(s, "hkf_slabs_load_map_coarser") and s.hkf_slabs_load_map_coarser(b"/nonexistent/x") == -1
    assert hasattr(H.App, "load_map_coarser") and hasattr(H.SlabsApp, "load_map_coarser")
    assert hasattr(K.Context, "merge_brick_store_halved")


def test_shift_is_arithmetic():
    keys = np.array([[-1, -3, 5], [-2, -4, 4], [0, 1, LO], [HI, HI - 1, -1]], np.int32)
    got = K.halved_brick_keys(keys)
    want = np.array([[0, 0, LO >> 1], [-1, -2, 2], [HI >> 1, HI >> 1, -1]], np.int32)
    want = want[np.lexsort((want[:, 0], want[:, 1], want[:, 2]))]
    assert np.array_equal(got, want) and np.array_equal(got, np_halved(keys))
    assert (LO >> 1) == -(1 << 19) and (HI >> 1) == (1 << 19) - 1


def test_halved_keys_against_numpy():
    keys = random_keys()
    want = np_halved(keys)
    assert len(want) < len(keys) and want[:, 0].min() == LO >> 1 and want[:, 0].max() == HI >> 1
    got = K.halved_brick_keys(keys)
    assert np.array_equal(got, want)
    o = got.astype(np.int64)
    word = ((o[:, 2] - LO) << 42) | ((o[:, 1] - LO) << 21) | (o[:, 0] - LO)
    assert np.all(np.diff(word) > 0)                               # unique and ascending by (z, y, x)
    perm = np.random.default_rng(1).permutation(len(keys))         # the order of the input plays no part
    assert np.array_equal(K.halved_brick_keys(np.ascontiguousarray(keys[perm])), want)
    twice = np.ascontiguousarray(np.concatenate([keys, keys[:10]]))  # nor does a key that occurs twice
    assert np.array_equal(K.halved_brick_keys(twice), want)


def test_cap_convention_and_refusals():
    keys = random_keys()
    want = np_halved(keys)
    n = len(want)
    assert raw(keys, None, 0) == n                                 # the count alone
    out = np.full((n + 2, 3), 77, np.int32)
    assert raw(keys, out, 5) == n and np.array_equal(out[:5], want[:5]) and np.all(out[5:] == 77)     # the first `cap`, nothing past them
    out[:] = 77
    assert raw(keys, out, n + 2) == n and np.array_equal(out[:n], want) and np.all(out[n:] == 77)     # a cap above the count
    assert raw(keys, None, 3) == -1                                # NULL out_keys with cap > 0
    assert raw(None, None, 0) == 0                                 # count 0: nothing is looked at
    assert K.load().kf_halved_brick_keys(2, None, None, 0) == -1   # NULL keys with count > 0
    for bad in ((HI + 1, 0, 0), (0, LO - 1, 0), (0, 0, 1 << 21), (-(1 << 31), 0, 0)):
        k = np.ascontiguousarray(np.array([[1, 2, 3], bad], np.int32))
        assert raw(k, None, 0) == -1, bad


def test_null_context_is_refused_without_a_device():
    lib = K.load()
    keys, t, w = np.zeros((1, 3), np.int32), np.zeros((1, 512), np.float32), np.ones((1, 512), np.float32)
    assert lib.kf_merge_brick_store_halved(None, 1, K._p(keys), K._p(t), K._p(w), None) == ARG
    assert lib.kf_merge_brick_store_halved(None, 0, None, None, None, None) == ARG
