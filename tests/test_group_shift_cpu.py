"""CPU-only: the moving volume over slab groups.  kf_group_shift_plan -- who sends which brick layers to whom for a z shift -- against a brute-force
numpy restatement of the rule; the argument refusals of the new entry points; header and binding agree on the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hybkinectfu_amd import group as G
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, HALO = 192, 8
NB = RES // 8
CUTS = {"uneven2": [0, 40, 192], "even3": [0, 64, 128, 192], "even8": list(range(0, 193, 24))}
DZS = [8, -8, 24, -24, 48, -48, 72, 192, -192, 0]


def stored(cuts, i, halo=HALO):
    hb = (halo + 7) // 8
    return max(0, cuts[i] // 8 - hb), min(NB, cuts[i + 1] // 8 + hb)


def brute_force(cuts, dz, halo=HALO):
    """per (receiver, layer): the owner that must send it.  For every stored destination layer p of every member: the source p + dz / 8 is
    stored there (nothing to send), lies outside the volume (empty), or belongs to exactly one owner"""
    sz = dz // 8 if dz >= 0 else -((-dz) // 8)
    owner = np.empty(NB, np.int64)
    for j in range(len(cuts) - 1):
        owner[cuts[j] // 8:cuts[j + 1] // 8] = j
    want = {}
    for to in range(len(cuts) - 1):
        b0, b1 = stored(cuts, to, halo)
        for p in range(b0, b1):
            q = p + sz
            if 0 <= q < NB and not (b0 <= q < b1):
                want[(to, q)] = int(owner[q])
    return want


@pytest.mark.parametrize("name", sorted(CUTS))
@pytest.mark.parametrize("dz", DZS)
def test_plan_equals_the_brute_force_rule(name, dz):
    cuts = CUTS[name]
    plan = G.shift_plan(RES, cuts, HALO, dz)
    assert plan is not None
    want = brute_force(cuts, dz)
    got = {}
    for frm, to, b0, b1 in plan:
        assert frm != to and b0 < b1
        assert cuts[frm] // 8 <= b0 and b1 <= cuts[frm + 1] // 8, (frm, b0, b1)       # never a layer the sender does not own
        for q in range(b0, b1):
            assert (to, q) not in got, (to, q)                                         # disjoint
            got[(to, q)] = frm
    assert got == want                                                                 # every need exactly once, from its owner
    assert plan == sorted(plan, key=lambda t: (t[1], t[2]))                            # by receiver, then by layer
    # each receiver's transfers tile one contiguous range: what kf_slab_shift_needs reports for it
    for to in range(len(cuts) - 1):
        mine = [t for t in plan if t[1] == to]
        assert all(a[3] == b[2] for a, b in zip(mine, mine[1:])), mine
    if dz == 0 or abs(dz) >= RES:
        assert plan == []


def test_plan_examples():
    """[0, 40, 192] with halo 8: member 0 stores brick layers [0, 6), member 1 [4, 24)"""
    assert G.shift_plan(RES, [0, 40, 192], 8, 8) == [(1, 0, 6, 7)]
    assert G.shift_plan(RES, [0, 40, 192], 8, -8) == [(0, 1, 3, 4)]
    assert G.shift_plan(RES, [0, 40, 192], 8, 48) == [(1, 0, 6, 12)]                   # member 0's whole content arrives from member 1
    assert G.shift_plan(RES, [0, 40, 192], 8, -48) == [(0, 1, 0, 4)]                   # member 1's layers [4, 10) take [-2, 4): only [0, 4) exist
    assert G.shift_plan(RES, [0, 64, 128, 192], 8, 72)[0:2] == [(1, 0, 9, 16), (2, 0, 16, 18)]     # wider than a slab: one feed from two owners
    assert G.shift_plan(RES, [0, 192], 8, 24) == []                                    # a whole-volume member needs nothing


def test_plan_refuses_bad_arguments():
    lib = G.load()
    good = (C.c_uint32 * 3)(0, 40, 192)
    out = (G.Transfer * 8)()
    assert lib.kf_group_shift_plan(192, 2, good, 8, 8, out, 8) == 1
    assert lib.kf_group_shift_plan(192, 2, good, 8, 8, None, 0) == 1                   # counting alone
    assert lib.kf_group_shift_plan(192, 2, good, 8, 8, None, 8) == -1
    assert lib.kf_group_shift_plan(192, 2, None, 8, 8, out, 8) == -1
    assert lib.kf_group_shift_plan(192, 2, good, 8, 4, out, 8) == -1                   # no whole bricks
    assert lib.kf_group_shift_plan(192, 2, good, 8, -12, out, 8) == -1
    assert lib.kf_group_shift_plan(190, 2, good, 8, 8, out, 8) == -1
    assert lib.kf_group_shift_plan(0, 2, good, 8, 8, out, 8) == -1
    assert lib.kf_group_shift_plan(192, 0, good, 8, 8, out, 8) == -1
    for bad in ([8, 40, 192], [0, 40, 184], [0, 44, 192], [0, 40, 40], [0, 96, 40]):
        arr = (C.c_uint32 * len(bad))(*bad)
        assert lib.kf_group_shift_plan(192, len(bad) - 1, arr, 8, 8, out, 8) == -1, bad
        assert G.shift_plan(192, bad, 8, 8) is None


def test_null_handles_are_refused():
    lib, glib = K.load(), G.load()
    a, b = C.c_uint32(), C.c_uint32()
    o = (C.c_int32 * 3)()
    assert lib.kf_slab_layer_bytes(None) == 0
    assert lib.kf_slab_shift_needs(None, 8, C.byref(a), C.byref(b)) == 1001
    assert lib.kf_slab_pack_layers(None, 0, 1, None) == 1001
    assert lib.kf_slab_needs(192, 0, 48, 8, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (6, 7)
    for bad in ((192, 0, 48, 4), (190, 0, 48, 8), (192, 4, 48, 8), (192, 48, 48, 8), (192, 0, 200, 8)):
        assert lib.kf_slab_needs(*bad, C.byref(a), C.byref(b)) == 1001, bad
    assert lib.kf_slab_needs(192, 0, 48, 8, None, C.byref(b)) == 1001
    assert lib.kf_shift_slab(None, 8, 0, 0, None, 0, 0) == 1001
    assert glib.kf_group_shift_volume(None, 8, 0, 0) == G.ERR_ARG
    assert glib.kf_group_raycast(None) == G.ERR_ARG
    assert glib.kf_group_volume_origin(None, o) == G.ERR_ARG
    slabs = C.CDLL(os.path.join(K.PKG_DIR, "libhybkf_slabs.so"))
    for name in ("hkf_slabs_shift_volume", "hkf_slabs_volume_origin", "hkf_slabs_set_recentre", "hkf_slabs_configure_traj", "hkf_slabs_process_frame_stamped"):
        assert hasattr(slabs, name), name
    slabs.hkf_slabs_shutdown()
    assert slabs.hkf_slabs_shift_volume(8, 0, 0) == -1 and slabs.hkf_slabs_volume_origin(o) == -1 and slabs.hkf_slabs_set_recentre(C.c_float(0.3)) == -1


def test_headers_and_bindings_agree_on_the_new_symbols():
    def declared(header, prefix):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, txt))
    new_group = {"kf_group_shift_plan", "kf_group_shift_volume", "kf_group_raycast", "kf_group_volume_origin"}
    new_ctx = {"kf_slab_layer_bytes", "kf_slab_shift_needs", "kf_slab_needs", "kf_slab_pack_layers", "kf_shift_slab"}
    assert new_group <= declared("hybkf_group.h", "kf_group_") and new_group <= set(G.SYMBOLS)
    assert new_ctx <= declared("hybkf.h", "kf_") and new_ctx <= set(K.SYMBOLS)
    for name in new_group:
        assert hasattr(G.load(), name), name
    for name in new_ctx:
        assert hasattr(K.load(), name), name
    assert C.sizeof(G.Transfer) == 16
    for m in ("shift_volume", "raycast", "volume_origin"):
        assert hasattr(G.Group, m), m
    for m in ("shift_slab", "pack_layers", "slab_shift_needs", "slab_layer_bytes"):
        assert hasattr(K.Context, m), m
