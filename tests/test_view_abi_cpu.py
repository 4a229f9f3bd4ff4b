"""CPU-only: the viewer-frame entry points exist at every layer (header, binding, the three libraries), refuse a null context, a bad mode and an
empty camera before they touch a device, and the numpy restatement of the byte formulas (view_expect.py), run on the oracle's maps of the
analytic volumes at the ragged camera, gives pictures with something in them -- the inputs the GPU test compares byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import raycast_scenarios as R
import view_expect as V
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kf_render_view", "kf_view_model_maps", "kf_view_size", "kf_view_device", "kf_read_view"]
ERR_ARG = 1001


def test_names_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name in ("KF_VIEW_NORMALS = 0", "KF_VIEW_SHADED = 1", "KF_VIEW_COLOR = 2"):
        assert name in txt, name
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", txt))
    K.build()
    lib = K.load()
    for name in NAMES:
        assert name in declared, name
        assert name in K.SYMBOLS, name
        assert hasattr(lib, name), name
    for method in ("render_view", "view_model_maps", "read_view", "view_device", "view_size"):
        assert callable(getattr(K.Context, method))
    assert (K.VIEW_NORMALS, K.VIEW_SHADED, K.VIEW_COLOR) == (0, 1, 2) == (V.VIEW_NORMALS, V.VIEW_SHADED, V.VIEW_COLOR)


def test_host_libraries_export_the_views():
    h = H.load()
    assert hasattr(h, "hkf_app_render_view") and hasattr(h, "hkf_app_view_model_maps")
    assert callable(H.App.render_view) and callable(H.App.view_model_maps)
    slabs = C.CDLL(os.path.join(K.PKG_DIR, "libhybkf_slabs.so"))
    assert hasattr(slabs, "hkf_slabs_view_model_maps")
    assert slabs.hkf_slabs_view_model_maps(0, None, C.c_size_t(0)) == -1          # no group: refused before anything else
    assert h.hkf_app_view_model_maps(0, None, C.c_size_t(0)) == -1
    assert h.hkf_app_render_view(0, None, 8, 8, C.c_float(4), C.c_float(4), C.c_float(8), C.c_float(8), None, C.c_size_t(0)) == -1


def test_argument_errors_come_before_any_device_call():
    """a null context, a mode outside the three and a camera without pixels are refused on a machine without a GPU: no HIP call is reached.  The
    bad-mode and bad-camera checks do not look into the context, so a block of zeros stands in for one."""
    lib = K.load()
    lib.kf_view_device.restype = C.c_void_p
    cam, rp = K.camera(*R.RAGGED), K.RaycastParams(0.1)
    near, far = C.c_float(0.3), C.c_float(4.0)
    n = C.c_uint32()
    buf = (C.c_uint8 * 16)()
    assert lib.kf_render_view(None, K.VIEW_NORMALS, None, C.byref(cam), C.byref(rp), near, far, None, None) == ERR_ARG
    assert lib.kf_view_model_maps(None, K.VIEW_NORMALS) == ERR_ARG
    assert lib.kf_view_size(None, C.byref(n), C.byref(n)) == ERR_ARG
    assert lib.kf_read_view(None, buf, C.c_size_t(16)) == ERR_ARG
    assert lib.kf_view_device(None) is None
    fake = (C.c_uint8 * (1 << 20))()                                              # all zeros; never dereferenced by the checks below
    for mode in (-1, 3, 255):
        assert lib.kf_render_view(fake, mode, None, C.byref(cam), C.byref(rp), near, far, None, None) == ERR_ARG, mode
        assert lib.kf_view_model_maps(fake, mode) == ERR_ARG, mode
    for bad in ((0, 152), (200, 0), (0, 0), (4097, 16), (16, 4097)):
        c = K.camera(bad[0], bad[1], *R.RAGGED[2:])
        assert lib.kf_render_view(fake, K.VIEW_SHADED, None, C.byref(c), C.byref(rp), near, far, None, None) == ERR_ARG, bad
    zero_f = K.camera(200, 152, 99.5, 75.5, 0.0, 164.0)
    assert lib.kf_render_view(fake, K.VIEW_SHADED, None, C.byref(zero_f), C.byref(rp), near, far, None, None) == ERR_ARG
    assert lib.kf_render_view(fake, K.VIEW_SHADED, None, None, C.byref(rp), near, far, None, None) == ERR_ARG
    assert lib.kf_render_view(fake, K.VIEW_SHADED, None, C.byref(cam), None, near, far, None, None) == ERR_ARG


# ---- the pictures the GPU test compares have something in them ------------------------------------------------------------------------------------
def _oracle(vid):
    vol = next(v for v in R.VOLUMES if v[0] == vid)
    ovol = R.oracle_volume(vol, R.volume_data(vol))
    return vol, ovol, [c for c in R.calls(vol) if c[1] == R.RAGGED]


SPARSE = ("far", "axes-x", "axes-y") + R.ZERO_HIT_VIEWS


def test_helper_on_the_oracles_maps_a104():
    """the conditions of the issue ("Inputs checked on the CPU") on a104 at RAGGED: >= 4600 hits, >= 200 grey levels and >= 750 normal triples per
    view outside the sparse ones; every non-hit NORMALS byte is 127; the zero-hit views are all background"""
    vol, ovol, calls = _oracle("a104")
    assert len(calls) == len(R.views(vol[2], vol[1]))
    for call in calls:
        key, _, view, pose, _, _ = call
        m = R.oracle_maps(vol, ovol, call)
        hit = m["v"][..., 3] == 1.0
        nrm = V.view_bytes(V.VIEW_NORMALS, m["v"], m["n"])
        shd = V.view_bytes(V.VIEW_SHADED, m["v"], m["n"], eye=pose[:3, 3])
        assert np.array_equal(nrm[..., 3] == 255, hit) and np.array_equal(shd[..., 3] == 255, hit), key
        assert np.all(nrm[~hit][:, :3] == 127) and np.all(shd[~hit] == 0), key
        assert np.all(shd[hit][:, 0] >= 32), key
        if view in R.ZERO_HIT_VIEWS:
            assert not hit.any(), key
        if view not in SPARSE:
            assert int(hit.sum()) >= 4600, (key, int(hit.sum()))
            assert len(np.unique(shd[hit][:, 0])) >= 200, (key, len(np.unique(shd[hit][:, 0])))
            assert len(np.unique(nrm[hit][:, :3], axis=0)) >= 750, (key, len(np.unique(nrm[hit][:, :3], axis=0)))


def test_helper_on_the_oracles_maps_c64():
    """c64: every listed view with a background has 5 to 183 pixels with a colour and no normal, and the COLOR picture carries them.  (axes-y
    looks along +y from inside the volume: all 30 400 pixels are hits in the oracle's maps, so it cannot have such a pixel -- asserted as that.)"""
    vol, ovol, calls = _oracle("c64")
    assert len(calls) == 7
    for call in calls:
        m = R.oracle_maps(vol, ovol, call)
        hit = m["v"][..., 3] == 1.0
        col = V.view_bytes(V.VIEW_COLOR, m["v"], m["n"], rgb=m["rgb"])
        lone = (m["rgb"].astype(np.int32).sum(axis=-1) > 0) & ~hit
        if call[2] == "axes-y":
            assert hit.all() and int(lone.sum()) == 0, (call[0], int(hit.sum()))
        else:
            assert 5 <= int(lone.sum()) <= 183, (call[0], int(lone.sum()))
        assert np.all(col[lone][:, 3] == 0) and np.all(col[lone][:, :3].astype(np.int32).sum(axis=-1) > 0), call[0]
        assert np.array_equal(col[..., :3], m["rgb"]) and np.array_equal(col[..., 3] == 255, hit), call[0]
