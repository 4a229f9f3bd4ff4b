"""CPU-only: the ABI of relocalisation.  kf_map_score_poses, kf_map_score_poses_device, kf_map_pose_sums and kf_map_refine_poses are exported, bound,
declared with the argument lists of include/hybkf.h and refuse a NULL context without a device, writing nothing; kf_pose_score is 24 bytes; the Python
methods exist; the sums' layout feeds kf_align_step unchanged: a step from sums built here from rows with a known twist recovers the twist.  The host
shims answer -1 without an application and the slab shim always does; hkf_reloc_points and hkf_reloc_rank equal their numpy restatements exactly,
hkf_reloc_lattice within 1e-15 on R and 1e-13 on t (the tolerances of test_map_align_abi_cpu.py for exp); and the host functions run in a stand-alone program
with a main of its own (tests/map_reloc_main.cpp), built with AddressSanitizer + UBSan: nothing of it is loaded into Python."""
import ctypes as C
import os
import re

import numpy as np

import map_align_expect as A
import map_reloc_expect as R
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1001
SCORE = ["uint32_t n_points", "const float* %spoints", "uint32_t n_poses", "const double* %sposes", "float band", "kf_pose_score* %sscores"]
SUMS = ["uint32_t n_points", "const float* points", "uint32_t n_poses", "const double* poses", "const double* centres", "float gate", "double* sums"]
REFINE = ["uint32_t n_points", "const float* points", "uint32_t n_poses", "double* poses", "const double* centres", "const kf_refine_params* params",
          "struct kf_align_report* reports"]


def declared_args(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_header_and_binding():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name, want in (("kf_map_score_poses", [a % "" if "%s" in a else a for a in SCORE]), ("kf_map_score_poses_device", [a % "dev_" if "%s" in a else a for a in SCORE]),
                       ("kf_map_pose_sums", SUMS), ("kf_map_refine_poses", REFINE)):
        assert hasattr(lib, name) and name in K.SYMBOLS, name
        args = declared_args(header, name)
        assert args[0] == "kf_ctx* ctx" and args[1:] == want, (name, args)
        assert len(getattr(lib, name).argtypes) == len(want) + 1, name
    assert re.search(r"^typedef struct kf_pose_score \{ uint32_t n_obs, n_in, n_behind, n_free; uint64_t sum_q; \} kf_pose_score;", header, re.M)
    assert re.search(r"^typedef struct kf_refine_params \{ uint32_t max_iter, min_pairs; double eps_rot, eps_trans; float gate; \} kf_refine_params;", header, re.M)
    assert K.POSE_SCORE_DTYPE.itemsize == 24 and K.POSE_SCORE_DTYPE.fields["sum_q"][1] == 16
    assert C.sizeof(K.RefineParams) == 32 and K.RefineParams.gate.offset == 24 and C.sizeof(K.AlignReport) == 296
    for name in ("map_score_poses", "map_score_poses_device", "map_pose_sums", "map_refine_poses"):
        assert hasattr(K.Context, name), name


def test_pose_score_is_24_bytes_in_c(tmp_path):
    """the struct as a C compiler lays it out, from the header itself"""
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hybkf.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(kf_pose_score), '
                   'offsetof(kf_pose_score, sum_q), sizeof(kf_refine_params), offsetof(kf_refine_params, gate)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"24", b"16", b"32", b"24"]


def test_null_context_is_refused_without_a_device():
    lib, p = K.load(), K._p
    pts, poses, centres = np.ones((4, 3), np.float32), np.tile(np.eye(3, 4).reshape(1, 12), (2, 1)), np.zeros((2, 3))
    kept = poses.copy()
    sc, sums, reps = np.full(48, 7, np.uint8), np.full(58, 7.0), np.full(2 * C.sizeof(K.AlignReport), 7, np.uint8)
    par = K.RefineParams(5, 1, 1e-6, 1e-6, 1.0)
    for fn in (lib.kf_map_score_poses, lib.kf_map_score_poses_device):
        assert fn(None, 4, p(pts), 2, p(poses), 0.5, p(sc)) == ARG
        assert fn(None, 0, None, 0, None, float("nan"), None) == ARG
    assert lib.kf_map_pose_sums(None, 4, p(pts), 2, p(poses), p(centres), 1.0, p(sums)) == ARG
    assert lib.kf_map_refine_poses(None, 4, p(pts), 2, p(poses), p(centres), C.byref(par), p(reps)) == ARG
    assert (sc == 7).all() and (sums == 7).all() and (reps == 7).all() and np.array_equal(poses, kept)     # refused: nothing written


def test_the_sums_feed_kf_align_step():
    """rows J = (x cross g, g) with e = J . xi for a known small twist: the 29 sums in kf_map_pose_sums' layout, handed to kf_align_step, give xi back, and
    the pose moves by T(c) exp(xi) T(-c)"""
    rng = np.random.default_rng(7)
    x, g = rng.uniform(-20, 20, (200, 3)), rng.normal(size=(200, 3)) * 0.25
    J = np.concatenate([np.cross(x, g), g], axis=1)
    xi = np.array([2e-3, -1e-3, 1.5e-3, 0.05, -0.02, 0.03])
    e = J @ xi
    sums = np.array([np.sum(J[:, a] * J[:, b]) for a, b in A.TRI] + [np.sum(J[:, a] * e) for a in range(6)] + [np.sum(e * e), 200.0])
    centre = np.array([30.0, 31.0, 29.0])
    pose = A.xf_of(A.rotation(25.0, (1, -1, 2)), (12.0, 40.0, -7.0))
    got = K.align_step(sums, centre, pose)
    assert got is not None and np.allclose(got[1], xi, rtol=0, atol=1e-12)
    E, u = A.np_exp(xi)
    assert np.allclose(got[0], A.xf_of(E @ pose[:, :3], E @ (pose[:, 3] - centre) + centre + u), rtol=0, atol=1e-12)


def test_shims_without_an_application():
    h, s = H.load(), H.load_slabs()
    mm = np.full(16, 1000, np.uint16)
    rep = H.RelocReport()
    before = bytes(rep)
    par = H.reloc_params()
    assert (par.top, par.max_points, par.level, list(par.n), par.has_guess) == (16, 4096, -1, [2] * 6, 0)
    for name in ("hkf_app_relocalise", "hkf_reloc_points", "hkf_reloc_lattice", "hkf_reloc_rank", "hkf_reloc_defaults_get"):
        assert hasattr(h, name), name
    assert h.hkf_app_relocalise(K._p(mm), C.c_uint(3), C.byref(par), C.byref(rep)) == -1 and bytes(rep) == before
    assert s.hkf_slabs_relocalise(K._p(mm), C.c_uint(3), C.byref(par), C.byref(rep)) == -1 and bytes(rep) == before
    assert s.hkf_slabs_relocalise(None, C.c_uint(0), None, None) == -1
    for name in ("relocalise",):
        assert hasattr(H.App, name) and hasattr(H.SlabsApp, name), name


def test_host_functions_equal_numpy():
    rng = np.random.default_rng(11)
    # points: a 40 x 30 vertex map with holes, more and fewer valid vertices than asked for
    v = rng.uniform(-1, 1, (1200, 4)).astype(np.float32)
    v[:, 2] = rng.uniform(0.4, 3.0, 1200).astype(np.float32)
    v[rng.random(1200) < 0.3, 2] = 0
    cell = np.float32(2.0) / np.float32(64)
    for cap in (4096, 500, 1, 840):
        got, med = H.reloc_points(v, cell, cap)
        want, wmed = R.np_points(v, cell, cap)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)) and med == np.float32(wmed), cap
    assert len(H.reloc_points(np.zeros((64, 4), np.float32), cell, 100)[0]) == 0
    # rank: many ties
    sc = np.zeros(5000, K.POSE_SCORE_DTYPE)
    sc["n_obs"], sc["n_in"], sc["sum_q"] = rng.integers(0, 40, 5000), rng.integers(0, 20, 5000), rng.integers(0, 8, 5000)
    sc["n_in"] = np.minimum(sc["n_in"], sc["n_obs"])
    for min_obs, m in ((0, 16), (10, 1), (30, 5000), (39, 7), (41, 3)):
        got, e = H.reloc_rank(sc, min_obs, m)
        want, we = R.np_rank(sc, min_obs, m)
        assert e == we and np.array_equal(got, want), (min_obs, m)
    # lattice
    centre = A.xf_of(A.rotation(33.0, (2, -1, 3)), (120.5, -40.25, 77.0))
    for n, ts, rs in (((2, 2, 2, 2, 2, 2), 5.0, 0.06), ((1, 0, 2, 0, 3, 1), 3.5, 0.2), ((0, 0, 0, 0, 0, 0), 1.0, 1.0), ((1, 1, 1, 1, 1, 1), 4.0, 1e-6)):
        got, want = H.reloc_lattice(centre, n, ts, rs), R.np_lattice(centre, n, ts, rs)
        assert got.shape == want.shape == (int(np.prod([2 * k + 1 for k in n])), 3, 4)
        assert np.allclose(got[:, :, :3], want[:, :, :3], rtol=0, atol=1e-15) and np.allclose(got[:, :, 3], want[:, :, 3], rtol=0, atol=1e-13), n
        assert np.array_equal(got[len(got) // 2], centre)        # the zero offset
    assert H.reloc_lattice(centre, (5, 5, 5, 5, 5, 5), 1.0, 0.1) is None and H.reloc_lattice(centre, (1, 1, 1, -1, 1, 1), 1.0, 0.1) is None


def test_host_side_under_sanitizers(tmp_path):
    import subprocess
    exe = str(tmp_path / "map_reloc_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "host"), os.path.join(ROOT, "tests", "map_reloc_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map reloc ok", out.stdout[-3000:]
