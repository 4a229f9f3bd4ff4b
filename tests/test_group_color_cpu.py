"""CPU-only: the colour forms of the z-slab merge and of slab groups exist -- the libraries export every new name either header declares -- and
kf_group_validate_color accepts a coloured layout, refuses what it must, and leaves kf_group_validate's refusal of colour where it was."""
import ctypes as C
import os
import re

import pytest

from hybkinectfu_amd import group as G
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybkinectfu_amd")
CORE_NAMES = ["kf_set_rgb_device", "kf_raycast_volume_slab_cross_spec_color", "kf_slab_ray_normals_color", "kf_set_model_maps_rays_color"]
GROUP_NAMES = ["kf_group_create_color", "kf_group_validate_color", "kf_group_frame_color", "kf_group_frame_members_color"]


def _declared(header, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, txt))


def _cfg(res=192, size=3.0, color=True, rgb=None):
    cfg = G.base_config(K.camera(*S.vga_camera()), res, size, has_color=color)
    if rgb is not None:
        cfg.rgb_camera = rgb
    return cfg


def test_headers_declare_the_colour_forms_and_the_libraries_export_them():
    core, group = _declared("hybkf.h", "kf_"), _declared("hybkf_group.h", "kf_group_")
    lib, glib = K.load(), G.load()
    for name in CORE_NAMES:
        assert name in core and name in K.SYMBOLS and hasattr(lib, name), name
    for name in GROUP_NAMES:
        assert name in group and name in G.SYMBOLS and hasattr(glib, name), name
    # every name either header declares with "color" or "rgb" in it is exported
    for name in sorted(n for n in core | group if "color" in n or "rgb" in n):
        assert hasattr(glib if name.startswith("kf_group_") else lib, name), name


def test_group_params_did_not_grow():
    assert C.sizeof(G.GroupParams) == 4 * 4 + C.sizeof(K.IcpParams) + C.sizeof(K.IntegrateParams) + C.sizeof(K.RaycastParams)


def test_validate_color_accepts_a_coloured_layout():
    p = G.stock_params()
    for angle in (True, False):
        assert G.validate_color_status(_cfg(), p, G.LOCAL, [0, 96, 192], angle_weight=angle) == 0
    assert G.validate_color_status(_cfg(), p, G.LOCAL, [0, 64, 128, 192], halo=16) == 0
    assert G.validate_color_status(_cfg(), p, G.RCCL_ALL, [0, 96, 192], devices=[0, 1]) == 0
    assert G.validate_color_status(_cfg(), p, G.RCCL_RANK, [0, 192], uid=bytes(G.UNIQUE_ID_BYTES), rank=0, world=1) == 0
    assert G.validate_color_status(_cfg(1024, 6.0), G.stock_params(trunc_max=6.0, integ_dist=6.0), G.LOCAL, list(range(0, 1025, 128)), halo=8) == 0


def test_validate_color_refuses_colourless_configs_and_empty_rgb_cameras():
    p = G.stock_params()
    assert G.validate_color_status(_cfg(color=False), p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG
    cfg = _cfg()
    cfg.has_color = 2                                                # the flag is 0 or 1
    assert G.validate_color_status(cfg, p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG
    cam = S.vga_camera()
    for cols, rows in ((0, 480), (640, 0), (0, 0)):
        assert G.validate_color_status(_cfg(rgb=K.camera(cols, rows, *cam[2:])), p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG, (cols, rows)
    assert G.validate_color_status(None, p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG
    assert G.validate_color_status(_cfg(), None, G.LOCAL, [0, 96, 192]) == G.ERR_ARG


@pytest.mark.parametrize("backend,cuts,kw", [
    (G.LOCAL, [0], {}), (G.LOCAL, [8 * i for i in range(17)] + [192], {}),                       # member count 0 and 17
    (G.LOCAL, [8, 96, 192], {}), (G.LOCAL, [0, 96, 184], {}), (G.LOCAL, [0, 96, 96, 192], {}), (G.LOCAL, [0, 100, 192], {}),
    (G.LOCAL, [0, 96, 192], dict(halo=4)),                                                       # thinner than pipeline.slab_halo_layers
    (G.LOCAL, [0, 96, 192], dict(devices=[0, 1])), (G.RCCL_ALL, [0, 96, 192], dict(devices=[0, 0])),
    (G.RCCL_RANK, [0, 96, 192], dict(uid=bytes(G.UNIQUE_ID_BYTES), rank=0, world=2)), (G.RCCL_RANK, [0, 192], dict(uid=None)),
    (7, [0, 96, 192], {}),
])
def test_validate_color_refuses_what_validate_refuses(backend, cuts, kw):
    p = G.stock_params()
    assert G.validate_status(_cfg(color=False), p, backend, cuts, **kw) == G.ERR_ARG             # (the colourless check refuses the layout ...)
    assert G.validate_color_status(_cfg(), p, backend, cuts, **kw) == G.ERR_ARG                  # (... and so does the colour check)


def test_colourless_entry_points_still_refuse_colour():
    p = G.stock_params()
    assert G.validate_status(_cfg(), p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG
    assert G.create_status(_cfg(), p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG
    assert G.validate_status(_cfg(color=False), p, G.LOCAL, [0, 96, 192]) == 0


def test_create_color_checks_before_any_device_call():
    lib = G.load()
    p, h = G.stock_params(), C.c_void_p()
    cuts = (C.c_uint32 * 3)(0, 96, 192)
    cfg = _cfg(color=False)
    assert lib.kf_group_create_color(C.byref(cfg), C.byref(p), 1, G.LOCAL, 2, cuts, None, 0, None, 0, 1, C.byref(h)) == G.ERR_ARG and not h
    cfg = _cfg()
    assert lib.kf_group_create_color(C.byref(cfg), C.byref(p), 1, G.LOCAL, 2, cuts, None, 0, None, 0, 1, None) == G.ERR_ARG
    assert lib.kf_group_frame_color(None, None, None, 0, 640, 480, 0) == G.ERR_ARG
    assert lib.kf_group_frame_members_color(None, None, None, 640, 480, 0) == G.ERR_ARG


def test_slab_shim_has_the_colour_switch_and_frame_entries():
    lib = C.CDLL(os.path.join(PKG, "libhybkf_slabs.so"))
    for name in ("hkf_slabs_configure_color", "hkf_slabs_process_frame_color", "hkf_slabs_enqueue_frame_color"):
        assert hasattr(lib, name), name
    assert lib.hkf_slabs_process_frame_color(None, None, 0, 0) == -1                             # no application
    # the switch is read by the next init: a bad layout still comes back as the group's argument error, before any HIP call
    lib.hkf_slabs_configure_color(1, 1)
    bad = (C.c_uint32 * 3)(0, 100, 192)
    assert lib.hkf_slabs_init(192, C.c_float(3.0), 640, 480, C.c_float(319.5), C.c_float(239.5), C.c_float(525.0), C.c_float(525.0), 0,
                              C.c_float(0), C.c_float(0), C.c_float(0), 0, G.LOCAL, 2, bad, None, 0) == G.ERR_ARG
    lib.hkf_slabs_configure_color(0, 1)
    lib.hkf_slabs_shutdown()
    host = C.CDLL(os.path.join(PKG, "libhybkf_host.so"))
    assert hasattr(host, "hkf_app_process_frame_color")
