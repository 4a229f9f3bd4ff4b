"""CPU-only: the parts of an indexed mesh and the drop of the small ones (include/hybkf.h has the rule), on the host side:
host/mesh_parts.hpp through hkf_mesh_from_soup + hkf_mesh_parts / hkf_mesh_drop_parts, and as a stand-alone program under the sanitizers.

The yardstick is the numpy restatement below (np_parts / np_drop): scipy's connected components over the face edges, labels by
np.minimum.at, sizes by np.bincount, compaction by boolean masks.  It is applied to the mesh read BEFORE the drop, and every comparison
is of bytes.  tests/test_gpu_mesh_parts.py runs the same soups (and larger ones) through the device against the same restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kf_mesh_parts", "kf_read_mesh_parts", "kf_mesh_drop_parts"]


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------
def np_parts(faces, n_v):
    """(labels, part_faces) per vertex: label = smallest vertex index of the vertex's part, part_faces = faces of that part (0: an orphan)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if n_v == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    rows = np.concatenate([faces[:, 0], faces[:, 0]])
    cols = np.concatenate([faces[:, 1], faces[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_v, n_v)).tocsr()
    n_comp, comp = connected_components(graph, directed=False)
    smallest = np.full(n_comp, n_v, np.int64)
    np.minimum.at(smallest, comp, np.arange(n_v))
    labels = smallest[comp]
    sizes = np.bincount(labels[faces[:, 0]], minlength=n_v)
    return labels.astype(np.uint32), sizes[labels].astype(np.uint32)


def np_drop(mesh, min_faces, largest_only):
    """the rule on a mesh dict (vertices, normals, colors, faces): (cleaned mesh, parts dropped, orphans dropped)"""
    n_v = len(mesh["vertices"])
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    labels, part_faces = np_parts(faces, n_v)
    thr = max(int(min_faces), 1)
    roots = np.nonzero((labels == np.arange(n_v)) & (part_faces > 0))[0]
    keep_part = part_faces[roots] >= thr
    if largest_only:
        only = np.zeros(len(roots), bool)
        if len(roots) and part_faces[roots].max() >= thr:
            only[np.argmax(part_faces[roots])] = True                 # the first maximum: roots ascend, a tie goes to the smallest label
        keep_part &= only
    keep_label = np.zeros(n_v + 1, bool)
    keep_label[roots[keep_part]] = True
    keep_v = keep_label[labels] if n_v else np.zeros(0, bool)
    keep_f = keep_v[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    new_id = np.cumsum(keep_v) - 1
    out = dict(vertices=mesh["vertices"][keep_v], normals=mesh["normals"][keep_v],
               colors=mesh["colors"][keep_v] if len(mesh["colors"]) == n_v else mesh["colors"],
               faces=new_id[faces[keep_f]].astype(np.uint32).reshape(-1, 3))
    return out, int(len(roots) - keep_part.sum()), int((part_faces == 0).sum())


def same_bytes(got, want, what=""):
    for k in ("vertices", "normals", "colors", "faces"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, k, g.shape, w.shape)


# ---- soups: vertices on a 0.01 lattice, so that the 1e-4 weld merges equal positions only ------------------------------------------------------
def soup_of(tri_xyz, colored=False):
    """(n, 3, 3) lattice coordinates (integers) -> triangles of lib.TRI_DTYPE; colours are a function of the position"""
    p = np.asarray(tri_xyz, np.float64).reshape(-1, 3, 3)
    s = np.zeros(len(p), K.TRI_DTYPE)
    s["v"]["pos"] = (p * 0.01).astype(np.float32)
    if colored:
        q = np.rint(p).astype(np.int64)
        s["v"]["color"] = np.stack([(q[..., 0] * 7 + q[..., 1]) % 256, (q[..., 1] * 5 + 3) % 256, (q[..., 2] + q[..., 0] * 3) % 256], -1).astype(np.float32) / 255
    return s


def fan(k, x0, y0, z0=0):
    """k faces around a centre: k + 2 vertices, one part"""
    c = (x0, y0, z0)
    rim = [(x0 + 1 + i, y0 + 2 + (i % 2), z0) for i in range(k + 1)]     # no three of a face's points on one line
    return [(c, rim[i], rim[i + 1]) for i in range(k)]


def strip(n, x0=0, y0=0, z0=0):
    """n triangles in one strip: n + 2 vertices, one part"""
    pt = lambda i: (x0 + i // 2, y0 + i % 2, z0)
    return [(pt(i), pt(i + 1), pt(i + 2)) for i in range(n)]


def contacts_vertex():
    return [((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((0, 0, 0), (-1, 0, 0), (0, -1, 0))]


def contacts_edge():
    return [((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((1, 0, 0), (1, 1, 0), (0, 1, 0)), ((50, 50, 5), (51, 50, 5), (50, 51, 5))]


def fans_1_to_6():
    t = []
    for k in range(1, 7):
        t += fan(k, 0, 10 * k)
    return t


def interleaved():
    a, b = strip(6, 0, 0, 0), strip(6, 0, 0, 9)
    return [x for pair in zip(a, b) for x in pair]


def many_singles(n_single=5000, n_strip=200):
    t = [((4 * (j % 100), 4 * (j // 100), 0), (4 * (j % 100) + 1, 4 * (j // 100), 0), (4 * (j % 100), 4 * (j // 100) + 1, 0)) for j in range(n_single // 2)]
    t += strip(n_strip, 0, 0, 7)
    t += [((4 * (j % 100), 4 * (j // 100), 20), (4 * (j % 100) + 1, 4 * (j // 100), 20), (4 * (j % 100), 4 * (j // 100) + 1, 20)) for j in range(n_single - n_single // 2)]
    return t


def two_equal_strips():
    return strip(40, 0, 0, 0) + [((9, 9, 3), (10, 9, 3), (9, 10, 3))] + strip(40, 0, 0, 5)


def orphan_soup():
    """a sliver whose first two vertices the weld merges (2e-5 apart: one cell): the face goes as degenerate, its third vertex stays, unnamed"""
    s = soup_of([((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, 0, 0), (30, 30, 30)), ((1, 0, 0), (1, 1, 0), (0, 1, 0))])
    s["v"]["pos"][1, 1, 0] += np.float32(2e-5)
    return s


def ordered(tris, order):
    tris = np.asarray(tris, np.int64).reshape(-1, 3, 3)
    if order == "descending":
        return tris[::-1]
    if order == "permuted":
        return tris[np.random.RandomState(7).permutation(len(tris))]
    return tris


# name -> (soup, colour, [(min_faces, largest_only), ...]); the device test adds the large ones
def small_cases():
    return {
        "contacts_vertex": (soup_of(contacts_vertex()), False, [(0, False), (2, False), (3, False)]),
        "contacts_edge": (soup_of(contacts_edge()), False, [(2, False), (1, False), (0, True)]),
        "threshold": (soup_of(fans_1_to_6()), False, [(3, False), (4, False), (6, True), (7, True), (7, False)]),
        "threshold_color": (soup_of(fans_1_to_6(), True), True, [(3, False), (4, False)]),
        "interleaved": (soup_of(interleaved()), False, [(0, True), (6, False), (7, False)]),
        "strip_ascending": (soup_of(ordered(strip(9000), "ascending")), False, [(9000, False), (9001, False)]),
        "strip_descending": (soup_of(ordered(strip(9000), "descending")), False, [(1, True)]),
        "strip_permuted": (soup_of(ordered(strip(9000), "permuted")), False, [(1, True)]),
        "many": (soup_of(many_singles()), False, [(0, True), (2, False), (201, False)]),
        "tie": (soup_of(two_equal_strips()), False, [(0, True), (40, True), (41, True)]),
        "orphan": (orphan_soup(), False, [(1, False), (0, False)]),
    }


CASES = small_cases()
RULES = [(name, mf, lo) for name, (_, _, rules) in CASES.items() for mf, lo in rules]


# ---- the layers exist ----------------------------------------------------------------------------------------------------------------------
def test_names_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", txt))
    K.build()
    lib = K.load()
    for name in NAMES:
        assert name in declared and name in K.SYMBOLS and hasattr(lib, name), name
    for method in ("mesh_parts", "read_mesh_parts", "mesh_drop_parts"):
        assert callable(getattr(K.Context, method))
    h = H.load()
    for name in ("hkf_app_set_min_part_faces", "hkf_mesh_drop_parts", "hkf_mesh_parts"):
        assert hasattr(h, name), name
    assert callable(H.App.set_min_part_faces) and callable(H.mesh_drop_parts) and callable(H.mesh_parts)


def test_null_context_is_an_argument_error():
    lib = K.load()
    n = C.c_uint32()
    assert lib.kf_mesh_parts(None, C.byref(n), C.byref(n), C.byref(n), C.byref(n)) == 1001
    assert lib.kf_read_mesh_parts(None, None, None) == 1001
    assert lib.kf_mesh_drop_parts(None, 3, 0, C.byref(n), C.byref(n)) == 1001


# ---- the host rule against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_labels_match_restatement(name):
    soup, color, _ = CASES[name]
    m = H.mesh_from_soup(soup, color)
    lab, cnt = H.mesh_parts(0)
    want_lab, want_cnt = np_parts(m["faces"], len(m["vertices"]))
    assert lab.tobytes() == want_lab.tobytes() and cnt.tobytes() == want_cnt.tobytes()
    if name.startswith("strip"):
        assert len(m["faces"]) == 9000 and len(m["vertices"]) == 9002 and not lab.any() and (cnt == 9000).all()
    if name == "orphan":
        assert (cnt == 0).sum() == 1 and len(m["faces"]) == 2
    if name == "contacts_vertex":
        assert len(m["vertices"]) == 5 and not lab.any()


@pytest.mark.parametrize("name,min_faces,largest_only", RULES)
def test_host_drop_matches_restatement(name, min_faces, largest_only):
    soup, color, _ = CASES[name]
    m = H.mesh_from_soup(soup, color)
    want, _, _ = np_drop(m, min_faces, largest_only)
    got = H.mesh_drop_parts(0, min_faces, largest_only)
    same_bytes(got, want, name)
    same_bytes(H.mesh_drop_parts(0, min_faces, largest_only), want, name + " again")          # a second identical drop is the identity


def test_rule_on_the_small_cases_by_hand():
    """the restatement itself, where the answer is plain"""
    m = H.mesh_from_soup(CASES["threshold"][0], False)                   # fans of 1 .. 6 faces, 3 .. 8 vertices
    for thr, faces, verts in ((3, 3 + 4 + 5 + 6, 5 + 6 + 7 + 8), (4, 4 + 5 + 6, 6 + 7 + 8)):
        out, pd, od = np_drop(m, thr, False)
        assert (len(out["faces"]), len(out["vertices"]), pd, od) == (faces, verts, thr - 1, 0)
    m = H.mesh_from_soup(CASES["tie"][0], False)
    out, pd, _ = np_drop(m, 0, True)
    assert pd == 2 and len(out["faces"]) == 40 and np.array_equal(out["vertices"], m["vertices"][:42])    # the first strip: the smaller label
    m = H.mesh_from_soup(CASES["interleaved"][0], False)
    lab, _ = np_parts(m["faces"], len(m["vertices"]))
    assert sorted(set(lab.tolist())) == [0, 3]                               # the two parts' vertices alternate as their faces do
    out, _, _ = np_drop(m, 0, True)
    assert np.array_equal(out["vertices"], m["vertices"][lab == 0]) and len(out["faces"]) == 6
    m = H.mesh_from_soup(CASES["orphan"][0], False)
    out, pd, od = np_drop(m, 1, False)
    assert (pd, od) == (0, 1) and len(out["vertices"]) == len(m["vertices"]) - 1 and len(out["faces"]) == len(m["faces"])


# ---- the header on its own, under the sanitizers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parts_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_parts") / "mesh_parts_main")
    pkg = os.path.join(ROOT, "hybkinectfu_amd")
    K.build()
    H.load()                                                            # libhybkf_host.so is there
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "mesh_parts_main.cpp"), "-o", exe, "-L", pkg, "-lhybkf_host", "-lhybkf", "-Wl,-rpath," + pkg])
    return exe


def _program_case(tris, min_faces, largest_only, extra_vertices=0):
    """an indexed mesh from lattice triangles (equal positions share a vertex, in first-use order) and its text for the program"""
    pts = np.asarray(tris, np.int64).reshape(-1, 3)
    verts, faces = np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    if len(pts):
        uniq, first, inv = np.unique(pts, axis=0, return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))                             # first-use order
        faces = rank[np.asarray(inv).reshape(-1)].reshape(-1, 3)
        verts = np.zeros((len(uniq), 3), np.int64)
        verts[rank] = uniq
    verts = np.concatenate([verts, np.full((extra_vertices, 3), 77) + np.arange(extra_vertices)[:, None]])       # orphans at the end
    text = "%d %d %d %d\n" % (len(verts), len(faces), min_faces, int(largest_only))
    text += "".join("%d %d %d\n" % tuple(v) for v in verts) + "".join("%d %d %d\n" % tuple(f) for f in faces)
    return text, verts, faces


def test_header_program_under_sanitizers(parts_program):
    specs = [(contacts_vertex(), 0, False, 0), (contacts_edge(), 2, False, 0), (fans_1_to_6(), 3, False, 2), (fans_1_to_6(), 4, False, 0),
             (fans_1_to_6(), 7, True, 1), (interleaved(), 0, True, 0), (ordered(strip(300), "permuted"), 1, True, 3), (many_singles(60, 20), 2, False, 0),
             (two_equal_strips(), 0, True, 0), ([], 0, False, 0), ([], 1, False, 4)]
    built = [_program_case(*s) for s in specs]
    out = subprocess.run([parts_program], input="".join(b[0] for b in built), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "mesh parts ok %d" % len(specs), out.stdout[-2000:]
    for i, ((_, mf, lo, _), (_, verts, faces)) in enumerate(zip(specs, built)):
        lab, cnt, dropped, kept, got_faces = [np.array(l.split()[1:], np.int64) for l in lines[5 * i:5 * i + 5]]
        want_lab, want_cnt = np_parts(faces, len(verts))
        assert np.array_equal(lab, want_lab) and np.array_equal(cnt, want_cnt), i
        idx = np.arange(len(verts), dtype=np.float32).reshape(-1, 1)
        want, pd, od = np_drop(dict(vertices=idx, normals=idx, colors=idx, faces=faces), mf, lo)
        assert dropped.tolist() == [pd, od], i
        assert np.array_equal(kept, want["vertices"].reshape(-1).astype(np.int64)), i
        assert np.array_equal(got_faces, want["faces"].reshape(-1).astype(np.int64)), i
