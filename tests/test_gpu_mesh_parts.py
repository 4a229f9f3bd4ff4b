"""The parts of the welded mesh on the device (csrc/meshparts.hip: kf_mesh_parts / kf_read_mesh_parts / kf_mesh_drop_parts; the rule stands in
include/hybkf.h) against the numpy restatement of tests/test_mesh_parts_cpu.py (np_parts / np_drop: scipy's connected components, np.minimum.at,
np.bincount, boolean masks), applied to the mesh read BEFORE the drop.  Every comparison is of bytes: vertices, normals, colours, faces, labels, sizes.
Soups go in with kf_write_triangles; their vertices lie on a 0.01 lattice, so the 1e-4 weld merges equal positions only."""

import numpy as np
import pytest

import test_gpu_shift as G
import test_mesh_parts_cpu as R
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K
from hybkinectfu_amd import scene as S
from test_mesh_parts_cpu import np_drop, np_parts, same_bytes

pytestmark = pytest.mark.gpu

SMALL_CAM = (160, 120, 79.5, 59.5, 131.25, 131.25)
ROUNDS = {}                                                          # case -> labelling rounds, printed for profiles/mesh_parts_c2.json


def parts_context(max_triangles, res=32, color=False):
    """a context for its triangle buffer alone"""
    return K.Context(K.camera(*SMALL_CAM), res, 3.0, levels=3, max_triangles=max_triangles, has_color=color)


@pytest.fixture
def shared():
    """one small context per test (the harness closes every context a test leaves open)"""
    ctx = parts_context(10000)
    yield ctx
    ctx.close()


def weld(ctx, soup, color=False):
    ctx.write_triangles(soup)
    ctx.weld_mesh(color, 1e-4)
    return ctx.read_mesh(color)


def check_labels(ctx, full, name=""):
    n_v = len(full["vertices"])
    want_lab, want_cnt = np_parts(full["faces"], n_v)
    n_parts, largest, orphans, rounds = ctx.mesh_parts()
    lab, cnt = ctx.read_mesh_parts()
    assert lab.tobytes() == want_lab.tobytes() and cnt.tobytes() == want_cnt.tobytes(), name
    roots = (want_lab == np.arange(n_v)) & (want_cnt > 0)
    assert (n_parts, largest, orphans) == (int(roots.sum()), int(want_cnt.max()) if n_v else 0, int((want_cnt == 0).sum())), name
    assert rounds <= n_v and (rounds >= 1) == (len(full["faces"]) > 0), (name, rounds)
    assert ctx.mesh_parts() == (n_parts, largest, orphans, rounds)                 # kept: asking again labels nothing anew
    return n_parts, largest, orphans, rounds


def check_case(ctx, soup, color, rules, name=""):
    """every rule on a fresh weld of the soup: labels, counts, the dropped mesh, the second drop, the counts of kf_mesh_counts, the soup itself"""
    info = None
    for min_faces, largest_only in rules:
        full = weld(ctx, soup, color)
        counts = ctx.mesh_counts()
        info = check_labels(ctx, full, name)
        want, pd, od = np_drop(full, min_faces, largest_only)
        assert ctx.mesh_drop_parts(min_faces, largest_only) == (pd, od), (name, min_faces, largest_only)
        same_bytes(ctx.read_mesh(color), want, (name, min_faces, largest_only))
        assert ctx.mesh_counts() == (len(want["vertices"]), len(want["faces"]), counts[2])
        assert ctx.mesh_drop_parts(min_faces, largest_only) == (0, 0)               # a second identical call changes nothing
        same_bytes(ctx.read_mesh(color), want, (name, "again"))
        assert np.array_equal(ctx.triangles().view(np.uint32), soup.view(np.uint32))   # the soup is only read
    return info


# ---- contacts, threshold, interleaved, many, tie, orphan, colour: the CPU module's soups ------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(R.CASES) if not n.startswith("strip")])
def test_small_soups_match_restatement(shared, name):
    soup, color, rules = R.CASES[name]
    ctx = shared if not color else parts_context(len(soup) + 8, color=True)
    n_parts, largest, orphans, _ = check_case(ctx, soup, color, rules, name)
    if name == "contacts_vertex":
        assert (n_parts, largest) == (1, 2)                       # two triangles meeting in one vertex only are one part
    if name == "contacts_edge":
        assert (n_parts, largest) == (2, 2)
        weld(ctx, soup)
        assert ctx.mesh_drop_parts(2, False) == (1, 0) and ctx.mesh_counts()[:2] == (4, 2)      # min_faces 2 drops the single
    if name == "threshold":
        for thr in (3, 4):                                        # >= is exact at the boundary: the fan of thr faces stays, the fan of thr - 1 goes
            weld(ctx, soup)
            assert ctx.mesh_drop_parts(thr, False) == (thr - 1, 0)
            assert sorted(set(ctx.read_mesh_parts()[1].tolist())) == list(range(thr, 7))
    if name == "threshold_color":
        full = weld(ctx, soup, True)
        assert len(np.unique(full["colors"].view(np.uint32), axis=0)) > 10         # real colours went through, and follow their vertices:
        ctx.mesh_drop_parts(4, False)
        kept = ctx.read_mesh(True)
        assert len(kept["vertices"]) == 6 + 7 + 8
        lut = {v.tobytes(): c.tobytes() for v, c in zip(full["vertices"], full["colors"])}
        assert all(lut[v.tobytes()] == c.tobytes() for v, c in zip(kept["vertices"], kept["colors"]))
        ctx.close()
    if name == "many":
        weld(ctx, soup)
        assert ctx.mesh_drop_parts(0, True) == (5000, 0) and ctx.mesh_counts()[:2] == (202, 200)   # largest_only keeps the strip
    if name == "tie":
        full = weld(ctx, soup)
        assert ctx.mesh_drop_parts(0, True) == (2, 0)
        assert ctx.read_mesh()["vertices"].tobytes() == full["vertices"][:42].tobytes()       # two equal strips: the smaller label stays
    if name == "orphan":
        full = weld(ctx, soup)
        assert orphans == 1 and ctx.mesh_drop_parts(1, False) == (0, 1)
        lone = np.nonzero(np_parts(full["faces"], len(full["vertices"]))[1] == 0)[0]
        assert ctx.read_mesh()["vertices"].tobytes() == np.delete(full["vertices"], lone, axis=0).tobytes()    # exactly that vertex went


# ---- strip: more than two scan chunks of faces and of vertices, in three soup orders ---------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_strip_is_one_part_in_any_soup_order(shared, order):
    soup, _, rules = R.CASES["strip_" + order]
    assert len(soup) == 9000 > 2 * 4096
    n_parts, largest, orphans, rounds = check_case(shared, soup, False, rules, order)
    assert (n_parts, largest, orphans) == (1, 9000, 0) and not shared.read_mesh_parts()[0].any()
    ROUNDS["strip_" + order] = rounds
    print("strip %s: 9000 faces, 9002 vertices, %d labelling rounds" % (order, rounds))


# ---- grid wrap: more faces and vertices than one pass of the walk's workgroups covers --------------------------------------------------------------
def test_more_faces_than_the_grid_walks_in_one_pass():
    n_fans = 100000
    base = np.array(R.fan(6, 0, 0), np.int64)                                             # (6, 3, 3)
    j = np.arange(n_fans)
    off = np.stack([10 * (j % 400), 5 * (j // 400), np.zeros(n_fans, np.int64)], -1)     # fans 8 x 4 lattice steps wide, 10 x 5 apart
    soup = R.soup_of((base[None] + off[:, None, None, :]).reshape(-1, 3, 3))
    assert len(soup) == 600000
    ctx = parts_context(len(soup))
    full = weld(ctx, soup)
    assert ctx.mesh_counts()[:2] == (800000, 600000)
    n_parts, largest, orphans, rounds = check_labels(ctx, full, "grid wrap")
    assert (n_parts, largest, orphans) == (n_fans, 6, 0)
    assert ctx.mesh_drop_parts(6, False) == (0, 0)                                      # everything left: the undropped mesh's bytes
    same_bytes(ctx.read_mesh(), full, "min_faces 6")
    assert ctx.mesh_drop_parts(7, False) == (n_fans, 0)                                 # nothing left: the empty mesh
    assert ctx.mesh_counts()[:2] == (0, 0)
    empty = ctx.read_mesh()
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3)
    assert ctx.mesh_parts() == (0, 0, 0, 0) and ctx.mesh_drop_parts(0, True) == (0, 0)
    print("grid wrap: 600000 faces, 800000 vertices, %d labelling rounds" % rounds)
    ctx.close()


# ---- a real surface: marching cubes of a sphere and three blobs --------------------------------------------------------------------------------------
def test_sphere_and_blobs_through_marching_cubes():
    res = 64
    z, y, x = np.meshgrid(*(np.arange(res, dtype=np.float32),) * 3, indexing="ij")
    balls = [((32, 32, 32), 20.3), ((8, 8, 8), 1.5), ((56, 10, 50), 1.5), ((12, 52, 9), 1.5)]
    t = np.full((res, res, res), 1e9, np.float32)
    for (cx, cy, cz), r in balls:
        t = np.minimum(t, np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - np.float32(r))
    t = np.clip(t, -1, 1).astype(np.float32)
    ctx = parts_context(400000, res=res)
    ctx.upload_volume(t, np.ones_like(t))
    ctx.marching_cubes(1.0e9)                                     # no threshold: every sign change counts
    soup = ctx.triangles()
    assert len(soup) > 5000
    ctx.weld_mesh(False, 1e-4)
    full = ctx.read_mesh()
    n_parts, largest, orphans, rounds = check_labels(ctx, full, "sphere")
    assert n_parts >= 2
    print("sphere + 3 blobs: %d faces, %d vertices, %d parts (largest %d faces), %d orphans, %d rounds" % (len(full["faces"]), len(full["vertices"]), n_parts, largest, orphans, rounds))
    want, pd, od = np_drop(full, 0, True)
    assert ctx.mesh_drop_parts(0, True) == (pd, od) and pd == n_parts - 1
    same_bytes(ctx.read_mesh(), want, "sphere")
    assert ctx.mesh_parts()[0] == 1 and ctx.mesh_parts()[2] == 0                  # exactly one part afterwards
    assert np.array_equal(ctx.triangles().view(np.uint32), soup.view(np.uint32))
    ctx.close()


# ---- bystander and state ---------------------------------------------------------------------------------------------------------------------------------
def test_state_reuse_and_determinism():
    import ctypes as C
    big, _, _ = R.CASES["many"]
    small, _, _ = R.CASES["threshold"]
    ctx = parts_context(len(big))
    lib, n = ctx.lib, C.c_uint32()
    assert lib.kf_mesh_parts(ctx.h, None, None, None, None) == 1002                # before any weld
    assert lib.kf_read_mesh_parts(ctx.h, None, None) == 1002
    assert lib.kf_mesh_drop_parts(ctx.h, 1, 0, None, None) == 1002
    ctx.weld_mesh(False, 1e-4)                                                    # an empty buffer: zeros
    assert ctx.mesh_parts() == (0, 0, 0, 0) and ctx.mesh_drop_parts(3, False) == (0, 0) and ctx.mesh_counts() == (0, 0, 0)
    assert lib.kf_read_mesh_parts(ctx.h, None, None) == 0
    full = weld(ctx, big)
    want, pd, od = np_drop(full, 2, False)
    assert ctx.mesh_drop_parts(2, False) == (pd, od)
    dropped = ctx.read_mesh()
    same_bytes(dropped, want, "big")
    assert lib.kf_mesh_parts(ctx.h, None, None, None, C.byref(n)) == 0             # any pointer may be NULL
    same_bytes(weld(ctx, big), full, "re-weld")                                   # the next weld gives the full mesh again
    small_full = weld(ctx, small)                                                 # a small mesh after a large one reuses the buffers
    want_small, pd, od = np_drop(small_full, 4, False)
    assert ctx.mesh_drop_parts(4, False) == (pd, od)
    same_bytes(ctx.read_mesh(), want_small, "small after big")
    full2 = weld(ctx, big)                                                        # ... and the large one again, after the buffers changed places
    same_bytes(full2, full, "big again")
    assert ctx.mesh_drop_parts(2, False)[0] == len(big) - 200
    same_bytes(ctx.read_mesh(), want, "big again, dropped")
    ctx.weld_release()
    assert lib.kf_mesh_parts(ctx.h, None, None, None, None) == 1002                # after kf_weld_release
    assert lib.kf_mesh_drop_parts(ctx.h, 1, 0, None, None) == 1002
    other = parts_context(len(big))                                               # the same mesh on a fresh context: the same bytes
    weld(other, big)
    lab_a, cnt_a = other.read_mesh_parts()
    other.mesh_drop_parts(2, False)
    same_bytes(other.read_mesh(), dropped, "fresh context")
    weld(ctx, big)
    lab_b, cnt_b = ctx.read_mesh_parts()
    assert lab_a.tobytes() == lab_b.tobytes() and cnt_a.tobytes() == cnt_b.tobytes()
    ctx.close(); other.close()


# ---- the host class ----------------------------------------------------------------------------------------------------------------------------------------
def _save(app, path):
    ok, nv, nf = app.save_mesh(path)
    assert ok
    return open(path, "rb").read(), H.app_mesh()


def test_host_class_drops_parts_on_both_weld_paths(tmp_path):
    """Scene S at 128^3 through the host class: saveMesh with setMinPartFaces under the device weld and under the host weld writes the same file, the
    restatement's mesh; with 0 it writes what it always wrote (the file of an application on which the setter was never called, and the mesh of
    kf_weld_mesh).  Once more for the map mesh after one window shift."""
    n_frames, n_min = 8, 40
    app = H.App(G.H_RES, G.H_SIZE, G.CAM, sdf_trunc=5 * G.H_SIZE / G.H_RES, integrate_dist=3.6, max_triangles=600000)
    app.set_brick_store(4096)
    for k in range(n_frames):
        assert app.process_frame(S.render_depth_mm(G.walk_pose(k, 20), G.CAM, G.H_SIZE), k, stamp=float(k)), k
    ctx = K.Context.borrow(app.ctx_handle(), K.camera(*G.CAM), G.H_RES, G.H_SIZE)
    p = lambda name: str(tmp_path / name)
    for stage in ("window", "map"):
        if stage == "map":
            assert app.shift_volume(48, 0, 0)
            app.set_map_mesh(True)
        assert app.generate_mesh() > 1000
        soup = ctx.triangles()
        app.set_device_weld(False)
        never, full = _save(app, p(stage + "_never.ply"))                          # the setter has not been called (window) / is off (map)
        n_parts = len(np.unique(np_parts(full["faces"], len(full["vertices"]))[0][full["faces"][:, 0]]))
        for n, largest_only in ((n_min, False), (0, True)):
            want, pd, od = np_drop(full, n, largest_only)
            print("host class, %s mesh: %d faces in %d parts; (%d, %s) drops %d parts, %d orphans, leaves %d faces" %
                  (stage, len(full["faces"]), n_parts, n, largest_only, pd, od, len(want["faces"])))
            app.set_min_part_faces(n, largest_only)
            app.set_device_weld(True)
            dev_file, dev_mesh = _save(app, p(stage + "_dev.ply"))
            assert ctx.mesh_counts()[:2] == (len(want["vertices"]), len(want["faces"]))      # saveMesh took the device path, drop included
            app.set_device_weld(False)
            host_file, host_mesh = _save(app, p(stage + "_host.ply"))
            assert dev_file == host_file
            same_bytes(dev_mesh, want, stage + " device")
            same_bytes(host_mesh, want, stage + " host")
            assert len(want["faces"]) > 0
        app.set_min_part_faces(0)
        app.set_device_weld(True)
        off_file, off_mesh = _save(app, p(stage + "_off.ply"))
        assert off_file == never
        same_bytes(off_mesh, full, stage + " off")
        assert np.array_equal(ctx.triangles().view(np.uint32), soup.view(np.uint32))
    app.close()
