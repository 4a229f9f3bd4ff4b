"""CPU-only: slab groups (include/hybkf_group.h) build, export what the header declares, keep RCCL out of libhybkf.so, and refuse every
invalid layout with an argument error before touching HIP or RCCL."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hybkinectfu_amd import group as G
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import pipeline as PL
from hybkinectfu_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hybkf_group.h")
PKG = os.path.join(ROOT, "hybkinectfu_amd")


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(kf_group_[a-z0-9_]+)\s*\(", txt)))


def _needed(path):
    out = subprocess.check_output(["readelf", "-d", path], text=True)
    return re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", out)


def test_build_produces_the_group_and_slab_libraries():
    import __graft_entry__
    __graft_entry__.build()
    for name in ("libhybkf_group.so", "libhybkf_slabs.so"):
        assert os.path.exists(os.path.join(PKG, name)), name
    assert "libhybkf_group.so" in _needed(os.path.join(PKG, "libhybkf_slabs.so"))
    assert any(n.startswith("librccl.so.1") for n in _needed(os.path.join(PKG, "libhybkf_group.so")))      # by SONAME


def test_libhybkf_has_no_rccl_dependency():
    assert not [n for n in _needed(os.path.join(PKG, "libhybkf.so")) if "rccl" in n]
    assert not [n for n in _needed(os.path.join(PKG, "libhybkf_host.so")) if "rccl" in n]


@pytest.mark.parametrize("lang,compiler", [("c", "gcc"), ("c++", "g++")])
def test_header_compiles_on_its_own(tmp_path, lang, compiler):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "hybkf_group.h"\nint probe(kf_group* g) { kf_group_params p; (void)p; return kf_group_synchronize(g); }\n')
    subprocess.check_call([compiler, "-x", lang, "-std=c11" if lang == "c" else "-std=c++17", "-Wall", "-Werror", "-pedantic",
                           "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_binding_lists_every_declared_function_and_the_library_exports_them():
    assert _declared() == sorted(G.SYMBOLS)
    lib = G.load()
    for name in _declared():
        assert hasattr(lib, name), name
    assert lib.kf_group_error_string(G.ERR_RCCL) == b"RCCL call failed"
    assert C.sizeof(G.GroupParams) == 4 * 4 + C.sizeof(K.IcpParams) + C.sizeof(K.IntegrateParams) + C.sizeof(K.RaycastParams)


def test_slab_library_exports_the_shim():
    lib = C.CDLL(os.path.join(PKG, "libhybkf_slabs.so"))
    for name in ("hkf_slabs_init", "hkf_slabs_shutdown", "hkf_slabs_process_frame", "hkf_slabs_enqueue_frame", "hkf_slabs_get_pose",
                 "hkf_slabs_generate_mesh", "hkf_slabs_save_mesh", "hkf_slabs_group"):
        assert hasattr(lib, name), name


def _cfg(res=192, size=3.0, color=False):
    return G.base_config(K.camera(*S.vga_camera()), res, size, has_color=color)


def test_halo_one_layer_thinner_than_the_pipeline_s_is_refused():
    """the thinnest halo the group accepts is pipeline.slab_halo_layers (rounded to a brick): one layer less is an argument error"""
    p = G.stock_params()
    for res, size in ((192, 3.0), (1024, 6.0), (512, 3.0), (128, 3.0)):
        halo = PL.slab_halo_layers(res, size, S.STOCK["raycast_increment_factor"] * S.STOCK["integrate_sdf_trunc"])
        assert G.create_status(_cfg(res, size), p, G.LOCAL, [0, res // 16 * 8, res], halo=halo - 1) == G.ERR_ARG, (res, size)


def test_validation_refuses_bad_layouts_without_a_gpu():
    p, cfg = G.stock_params(), _cfg()
    lib = G.load()
    h = C.c_void_p()
    cuts = (C.c_uint32 * 3)(0, 96, 192)
    # NULLs
    assert lib.kf_group_create(None, C.byref(p), G.LOCAL, 2, cuts, None, 0, None, 0, 1, C.byref(h)) == G.ERR_ARG
    assert lib.kf_group_create(C.byref(cfg), None, G.LOCAL, 2, cuts, None, 0, None, 0, 1, C.byref(h)) == G.ERR_ARG
    assert lib.kf_group_create(C.byref(cfg), C.byref(p), G.LOCAL, 2, None, None, 0, None, 0, 1, C.byref(h)) == G.ERR_ARG
    assert lib.kf_group_create(C.byref(cfg), C.byref(p), G.LOCAL, 2, cuts, None, 0, None, 0, 1, None) == G.ERR_ARG
    for fn in ("kf_group_destroy", "kf_group_synchronize", "kf_group_marching_cubes"):
        assert getattr(lib, fn)(None, *([C.c_float(0.0)] if fn == "kf_group_marching_cubes" else [])) == G.ERR_ARG, fn
    assert lib.kf_group_frame(None, None, 0, 640, 480, 0) == G.ERR_ARG
    assert lib.kf_group_unique_id(None) == G.ERR_ARG
    # member count: 0 and 17
    assert G.create_status(cfg, p, G.LOCAL, [0]) == G.ERR_ARG
    assert G.create_status(cfg, p, G.LOCAL, [8 * i for i in range(17)] + [192]) == G.ERR_ARG
    # cuts that do not tile the volume, do not rise, are not brick aligned
    for cuts in ([8, 96, 192], [0, 96, 184], [0, 96, 200], [0, 96, 96, 192], [0, 120, 96, 192], [0, 100, 192], [0, 96, 190]):
        assert G.create_status(cfg, p, G.LOCAL, cuts) == G.ERR_ARG, cuts
    # a halo thinner than pipeline.slab_halo_layers (8 layers at 192^3 @ 3 m)
    assert G.create_status(cfg, p, G.LOCAL, [0, 96, 192], halo=4) == G.ERR_ARG
    big = G.stock_params()
    big.raycast.ray_increment = 0.2                                  # 13 voxels per step at 192^3 @ 3 m: needs 15 -> 16 layers
    assert G.create_status(cfg, big, G.LOCAL, [0, 96, 192], halo=8) == G.ERR_ARG
    # colour
    assert G.create_status(_cfg(color=True), p, G.LOCAL, [0, 96, 192]) == G.ERR_ARG
    # LOCAL across two devices; RCCL_ALL with a repeated device
    assert G.create_status(cfg, p, G.LOCAL, [0, 96, 192], devices=[0, 1]) == G.ERR_ARG
    assert G.create_status(cfg, p, G.RCCL_ALL, [0, 96, 192], devices=[0, 0]) == G.ERR_ARG
    assert G.create_status(cfg, p, G.RCCL_ALL, [0, 64, 128, 192], devices=[0, 1, 0]) == G.ERR_ARG
    assert G.create_status(cfg, p, G.RCCL_ALL, [0, 96, 192]) == G.ERR_ARG             # (devices NULL: every member on base->device)
    # RCCL_RANK: one member per process, a unique id, rank < world
    uid = bytes(G.UNIQUE_ID_BYTES)
    assert G.create_status(cfg, p, G.RCCL_RANK, [0, 96, 192], uid=uid, rank=0, world=2) == G.ERR_ARG
    assert G.create_status(cfg, p, G.RCCL_RANK, [0, 192], uid=None, rank=0, world=1) == G.ERR_ARG
    assert G.create_status(cfg, p, G.RCCL_RANK, [0, 192], uid=uid, rank=2, world=2) == G.ERR_ARG
    # an unknown backend
    assert G.create_status(cfg, p, 7, [0, 96, 192]) == G.ERR_ARG


def test_slab_shim_refuses_bad_layouts():
    """hkf_slabs_init hands the group's argument errors back before any HIP call"""
    lib = C.CDLL(os.path.join(PKG, "libhybkf_slabs.so"))
    assert lib.hkf_slabs_init(192, C.c_float(3.0), 640, 480, C.c_float(319.5), C.c_float(239.5), C.c_float(525.0), C.c_float(525.0), 0,
                              C.c_float(0), C.c_float(0), C.c_float(0), 0, G.LOCAL, 17, None, None, 0) == G.ERR_ARG
    # colourless, brick-aligned, tiling: a bad explicit layout comes back as the group's argument error, before any HIP call
    bad = (C.c_uint32 * 3)(0, 100, 192)
    assert lib.hkf_slabs_init(192, C.c_float(3.0), 640, 480, C.c_float(319.5), C.c_float(239.5), C.c_float(525.0), C.c_float(525.0), 0,
                              C.c_float(0), C.c_float(0), C.c_float(0), 0, G.LOCAL, 2, bad, None, 0) == G.ERR_ARG
    two = (C.c_int32 * 2)(0, 1)
    assert lib.hkf_slabs_init(192, C.c_float(3.0), 640, 480, C.c_float(319.5), C.c_float(239.5), C.c_float(525.0), C.c_float(525.0), 0,
                              C.c_float(0), C.c_float(0), C.c_float(0), 0, G.LOCAL, 2, None, two, 0) == G.ERR_ARG
    lib.hkf_slabs_shutdown()


def test_rccl_rank_takes_this_rank_s_own_slab():
    """RCCL_RANK: each rank passes its own {z0, z1}; the ranks of a world tile the volume in rank order (kf_group_validate: the checks of
    kf_group_create without ncclCommInitRank, which would wait for the other ranks)"""
    p, cfg = G.stock_params(), _cfg()
    uid = bytes(G.UNIQUE_ID_BYTES)
    layout = [0, 40, 104, 192]                                       # a world-3 layout, uneven
    for r in range(3):
        assert G.validate_status(cfg, p, G.RCCL_RANK, layout[r:r + 2], uid=uid, rank=r, world=3) == 0, r
    assert G.validate_status(cfg, p, G.RCCL_RANK, [0, 96], uid=uid, rank=0, world=2) == 0
    assert G.validate_status(cfg, p, G.RCCL_RANK, [96, 192], uid=uid, rank=1, world=2) == 0
    assert G.validate_status(cfg, p, G.RCCL_RANK, [0, 192], uid=uid, rank=0, world=1) == 0
    for cuts, rank, world in (([96, 192], 0, 2),                     # rank 0 must start at 0
                              ([0, 96], 1, 2),                       # the last rank must end at the resolution
                              ([0, 96], 0, 1),                       # a world-1 rank owns the whole volume
                              ([0, 192], 1, 3), ([40, 192], 1, 3),   # a middle rank lies strictly inside
                              ([96, 96], 1, 2), ([100, 192], 1, 2), ([96, 200], 1, 2), ([0, 92], 0, 2)):
        assert G.validate_status(cfg, p, G.RCCL_RANK, cuts, uid=uid, rank=rank, world=world) == G.ERR_ARG, (cuts, rank, world)
    assert G.validate_status(cfg, p, G.RCCL_RANK, [96, 192], uid=None, rank=1, world=2) == G.ERR_ARG
    assert G.validate_status(cfg, p, G.RCCL_RANK, [96, 192], uid=uid, rank=1, world=25) == G.ERR_ARG          # more ranks than brick layers


def test_validate_and_create_share_one_check():
    """kf_group_validate and kf_group_create apply one check: valid LOCAL / RCCL_ALL layouts pass, the refused ones fail alike"""
    p, cfg = G.stock_params(), _cfg()
    assert G.validate_status(cfg, p, G.LOCAL, [0, 40, 192]) == 0
    assert G.validate_status(cfg, p, G.LOCAL, [0, 64, 128, 192], halo=16) == 0
    assert G.validate_status(cfg, p, G.RCCL_ALL, [0, 96, 192], devices=[0, 1]) == 0
    for args in ((G.LOCAL, [0, 100, 192], None), (G.LOCAL, [0, 96, 192], [0, 1]), (G.RCCL_ALL, [0, 96, 192], [1, 1])):
        assert G.validate_status(cfg, p, args[0], args[1], devices=args[2]) == G.ERR_ARG == G.create_status(cfg, p, args[0], args[1], devices=args[2])
