"""CPU-only: the merged view over slab groups exists at every layer -- both headers (which still compile on their own as C11 and C++17), the
three libraries, the bindings -- and kf_group_view_validate, which makes no HIP call, refuses what kf_group_render_view refuses."""
import ctypes as C
import os
import re
import subprocess

import pytest

import raycast_scenarios as R
from hybkinectfu_amd import group as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX_NAMES = ["kf_view_slab_cross", "kf_view_slab_normals", "kf_view_from_rays"]
GROUP_NAMES = ["kf_group_view_validate", "kf_group_render_view", "kf_group_view_size", "kf_group_view_device", "kf_group_read_view"]
NAN = float("nan")


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", txt))


@pytest.mark.parametrize("header", ["hybkf.h", "hybkf_group.h"])
@pytest.mark.parametrize("lang,compiler", [("c", "gcc"), ("c++", "g++")])
def test_headers_compile_on_their_own(tmp_path, header, lang, compiler):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    probe = {"hybkf.h": "int probe(kf_ctx* c) { return kf_view_from_rays(c, KF_VIEW_SHADED, 0, 0, 0, 0, 3, 0, 0); }",
             "hybkf_group.h": "int probe(kf_group* g) { return kf_group_render_view(g, KF_VIEW_SHADED, 0, 0, 0.f, 1.f, 0, 0); }"}[header]
    src.write_text('#include "%s"\n%s\n' % (header, probe))
    subprocess.check_call([compiler, "-x", lang, "-std=c11" if lang == "c" else "-std=c++17", "-Wall", "-Werror", "-pedantic",
                           "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_names_declared_listed_and_exported():
    K.build()
    lib, glib = K.load(), G.load()
    for name in CTX_NAMES:
        assert name in _declared("hybkf.h") and name in K.SYMBOLS and hasattr(lib, name), name
    for name in GROUP_NAMES:
        assert name in _declared("hybkf_group.h") and name in G.SYMBOLS and hasattr(glib, name), name
    for method in ("view_slab_cross", "view_slab_normals", "view_from_rays"):
        assert callable(getattr(K.Context, method)), method
    for method in ("render_view", "read_view", "view_size", "view_device"):
        assert callable(getattr(G.Group, method)), method
    assert callable(G.view_validate_status)
    # the sentences that called a free viewpoint over a group out of scope are gone
    for header in ("hybkf.h", "hybkf_group.h"):
        assert "out of scope" not in open(os.path.join(ROOT, "include", header)).read(), header
    assert "kf_group_render_view" in open(os.path.join(ROOT, "include", "hybkf.h")).read()


def test_slab_library_exports_render_view():
    slabs = C.CDLL(os.path.join(K.PKG_DIR, "libhybkf_slabs.so"))
    assert hasattr(slabs, "hkf_slabs_render_view")
    assert slabs.hkf_slabs_render_view(0, None, 8, 8, C.c_float(4), C.c_float(4), C.c_float(8), C.c_float(8), None, C.c_size_t(0)) == -1      # no group
    assert callable(H.SlabsApp.render_view)


def test_view_validate_refuses_without_a_gpu():
    ok = K.camera(*R.RAGGED)
    for color_group in (0, 1):
        for mode in (-1, 3):
            assert G.view_validate_status(color_group, mode, ok) == G.ERR_ARG, mode
        for cols, rows in ((0, 152), (200, 0), (4097, 152), (200, 4097)):
            assert G.view_validate_status(color_group, K.VIEW_SHADED, K.camera(cols, rows, *R.RAGGED[2:])) == G.ERR_ARG, (cols, rows)
        for cx, cy, fx, fy in ((99.5, 75.5, 0.0, 164.0), (99.5, 75.5, 164.0, 0.0), (99.5, 75.5, NAN, 164.0), (99.5, 75.5, 164.0, NAN),
                               (NAN, 75.5, 164.0, 164.0), (99.5, NAN, 164.0, 164.0)):
            assert G.view_validate_status(color_group, K.VIEW_NORMALS, K.camera(200, 152, cx, cy, fx, fy)) == G.ERR_ARG, (cx, cy, fx, fy)
        assert G.view_validate_status(color_group, K.VIEW_NORMALS, None) == G.ERR_ARG
    assert G.view_validate_status(0, K.VIEW_COLOR, ok) == G.ERR_STATE
    assert G.view_validate_status(1, K.VIEW_COLOR, ok) == 0


def test_view_validate_accepts_the_extreme_sizes():
    for color_group in (0, 1):
        for mode in (K.VIEW_NORMALS, K.VIEW_SHADED):
            assert G.view_validate_status(color_group, mode, K.camera(1, 1, 0.0, 0.0, 82.0, 82.0)) == 0
            assert G.view_validate_status(color_group, mode, K.camera(4096, 4096, 2047.5, 2047.5, 3000.0, 3000.0)) == 0


def test_null_arguments_come_before_any_device_call():
    lib, glib = K.load(), G.load()
    glib.kf_group_view_device.restype = C.c_void_p
    cam, rp = K.camera(*R.RAGGED), K.RaycastParams(0.1)
    near, far = C.c_float(0.3), C.c_float(4.0)
    n = C.c_uint32()
    buf = (C.c_uint8 * 16)()
    assert glib.kf_group_render_view(None, K.VIEW_NORMALS, None, C.byref(cam), near, far, None, None) == G.ERR_ARG
    assert glib.kf_group_view_size(None, C.byref(n), C.byref(n)) == G.ERR_ARG
    assert glib.kf_group_read_view(None, buf, C.c_size_t(16)) == G.ERR_ARG
    assert glib.kf_group_view_device(None) is None
    assert lib.kf_view_slab_cross(None, 0, None, C.byref(cam), C.byref(rp), near, far, buf, buf, buf) == G.ERR_ARG
    assert lib.kf_view_slab_normals(None, 0, None, C.byref(cam), C.byref(rp), near, far, buf, buf, buf, buf) == G.ERR_ARG
    assert lib.kf_view_from_rays(None, K.VIEW_NORMALS, None, C.byref(cam), buf, buf, 3, None, None) == G.ERR_ARG
    fake = (C.c_uint8 * (1 << 20))()                                              # all zeros; never dereferenced by the checks below
    assert lib.kf_view_from_rays(fake, K.VIEW_COLOR, None, C.byref(cam), buf, buf, 3, None, None) == G.ERR_ARG       # colour needs 4 words
    assert lib.kf_view_from_rays(fake, K.VIEW_SHADED, None, C.byref(cam), buf, buf, 5, None, None) == G.ERR_ARG
    assert lib.kf_view_from_rays(fake, 3, None, C.byref(cam), buf, buf, 3, None, None) == G.ERR_ARG
    assert lib.kf_view_from_rays(fake, K.VIEW_SHADED, None, C.byref(K.camera(0, 4, *R.RAGGED[2:])), buf, buf, 3, None, None) == G.ERR_ARG
