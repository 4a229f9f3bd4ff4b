"""CPU-only: the ABI and the host side of aligning two maps.  kf_align_brick_store and kf_align_step are exported, bound, declared and refuse what they must
without a device; the host shim's names and the Python methods exist and answer -1 / False without an application.  kf_align_step is compared with numpy's
float64 solve on the sums the restatement (map_align_expect.py) gives for the three analytic cases.  The header the step and the loop's turn live in
(csrc/align_step.h) also runs in a stand-alone program with a main of its own (tests/map_align_main.cpp), built with AddressSanitizer + UBSan: nothing of it
is loaded into Python; that program pins every verdict of the loop on crafted sums, and the same sequences go through the yardstick's loop here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_align_expect as E
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE = (32.0, 32.0, 32.0)


def test_symbols_exported_bound_and_declared():
    lib = K.load()
    header = open(os.path.join(ROOT, "include", "hybkf.h")).read()
    for name in ("kf_align_brick_store", "kf_align_step"):
        assert hasattr(lib, name) and name in K.SYMBOLS, name
    assert re.search(r"^int kf_align_brick_store\(kf_ctx\* ctx, uint32_t count, const int32_t\* keys,", header, re.M)
    assert re.search(r"^int kf_align_step\(const double sums\[29\], const double centre\[3\], double xf\[12\], double step\[6\]\);", header, re.M)
    assert len(lib.kf_align_brick_store.argtypes) == 8 and len(lib.kf_align_step.argtypes) == 4
    # the structs as the header lays them out: two uint32, then doubles
    assert C.sizeof(K.AlignParams) == 8 + 8 * 5 and C.sizeof(K.AlignReport) == 8 + 8 * (29 + 1 + 6)
    assert K.AlignParams.centre.offset == 24 and K.AlignReport.sums.offset == 8 and K.AlignReport.rms.offset == 240 and K.AlignReport.step.offset == 248
    assert re.search(r"typedef struct kf_align_params \{ uint32_t max_iter, min_pairs; double eps_rot, eps_trans; double centre\[3\]; \}", header)
    assert re.search(r"typedef struct kf_align_report \{ uint32_t iterations, verdict; double sums\[29\]; double rms; double step\[6\]; \}", header)
    for name, value in (("CONVERGED", 0), ("ITER_LIMIT", 1), ("FEW_PAIRS", 2), ("SINGULAR", 3)):
        assert re.search(r"^#define KF_ALIGN_%s %d$" % (name, value), header, re.M) and getattr(K, "ALIGN_" + name) == value == getattr(E, name)
    assert float(re.search(r"^#define KF_ALIGN_EPS_ROT_MIN (\S+)", header, re.M).group(1)) == E.EPS_ROT_MIN
    assert float(re.search(r"^#define KF_ALIGN_EPS_TRANS_MIN (\S+)", header, re.M).group(1)) == E.EPS_TRANS_MIN
    assert hasattr(K.Context, "align_brick_store") and hasattr(K, "align_step")


def test_argument_errors_without_a_device():
    lib = K.load()
    keys, t, w = np.zeros((1, 3), np.int32), np.zeros(512, np.float32), np.ones(512, np.float32)
    xf, p, rep = K.rigid_xf(np.eye(3, 4)), K.align_params(CENTRE), K.AlignReport()
    assert lib.kf_align_brick_store(None, 1, K._p(keys), K._p(t), K._p(w), xf, C.byref(p), C.byref(rep)) == 1001
    assert lib.kf_align_brick_store(None, 0, None, None, None, None, None, None) == 1001
    sums, step = (C.c_double * 29)(), (C.c_double * 6)()
    c = (C.c_double * 3)(*CENTRE)
    assert lib.kf_align_step(None, c, xf, step) != 0 and lib.kf_align_step(sums, None, xf, step) != 0
    assert lib.kf_align_step(sums, c, None, step) != 0 and lib.kf_align_step(sums, c, xf, None) != 0
    assert lib.kf_align_step(sums, c, xf, step) != 0             # a zero matrix
    assert list(xf) == np.eye(3, 4).reshape(12).tolist() and list(step) == [0.0] * 6


def test_shims_without_an_application():
    h = H.load()
    m, found = np.eye(4, dtype=np.float32), np.zeros(16, np.float32)
    assert hasattr(h, "hkf_app_align_map")
    assert h.hkf_app_align_map(b"/nonexistent/x", m.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p), None) == -1
    s = H.load_slabs()                                            # the slab class refuses: the store stays a single-GPU feature
    assert hasattr(s, "hkf_slabs_align_map")
    assert s.hkf_slabs_align_map(b"/nonexistent/x", m.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p), None) == -1
    assert hasattr(H.App, "align_map") and hasattr(H.SlabsApp, "align_map")


_SUMS = {}


def sums_at_identity(name):
    if name not in _SUMS:
        _SUMS[name] = E.np_sums(E.analytic_map(), E.analytic_map(name), np.eye(3, 4), CENTRE)[0]
    return _SUMS[name]


@pytest.mark.parametrize("name", list(E.MOVES))
def test_step_against_numpy(name):
    """the step from the restatement's own sums at the identity: against numpy's float64 solve to 64 cond(A) 2^-53 |xi| -- Cholesky and LU are both backward
    stable, each solution within a small multiple of cond(A) 2^-53 of the exact one; 64 leaves room for the constants of a 6 x 6 system -- and the updated
    transform against the restatement's update of that step"""
    sums = sums_at_identity(name)
    assert sums[28] >= 10000
    A, b = E.matrix_of(sums)
    want = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    got = K.align_step(sums, CENTRE, np.eye(3, 4))
    assert got is not None
    xf, xi = got
    print(name, "cond", cond, "|xi|", np.linalg.norm(want), "difference", np.linalg.norm(xi - want), "bound", 64 * cond * 2.0 ** -53 * np.linalg.norm(want))
    assert np.linalg.norm(xi - want) <= 64 * cond * 2.0 ** -53 * np.linalg.norm(want)
    ex, u = E.np_exp(xi)
    c = np.asarray(CENTRE)
    assert np.allclose(xf[:, :3], ex, rtol=0, atol=1e-15) and np.allclose(xf[:, 3], ex @ (0 - c) + c + u, rtol=0, atol=1e-13)
    assert np.max(np.abs(xf[:, :3].T @ xf[:, :3] - np.eye(3))) < 1e-15


def test_step_refuses_a_zero_matrix_and_a_zero_pivot():
    sums = sums_at_identity("5deg").copy()
    assert K.align_step(np.zeros(29), CENTRE, np.eye(3, 4)) is None
    z = sums.copy()
    for k, (a, b) in enumerate(E.TRI):
        if a == 2 or b == 2:
            z[k] = 0.0                                            # row and column 2: the third pivot is exactly 0
    assert K.align_step(z, CENTRE, np.eye(3, 4)) is None
    n = sums.copy()
    n[0] = -n[0]
    assert K.align_step(n, CENTRE, np.eye(3, 4)) is None
    assert K.align_step(sums, CENTRE, np.eye(3, 4)) is not None


def test_restatement_recovers_the_moves():
    """the yardstick by itself, on the smallest move: its loop converges from the identity onto X^-1 (the three cases' figures: test_gpu_map_align.py)"""
    truth = E.inverse(E.move("2deg"))
    xf, verdict, it, sums, _ = E.np_align(E.analytic_map(), E.analytic_map("2deg"), np.eye(3, 4), CENTRE)
    err = E.errors(xf, truth, CENTRE)
    print("2deg: iterations", it, "errors", err, "pairs", sums[28])
    assert verdict == E.CONVERGED and it <= 8 and err[0] < 0.02 and err[1] < 1e-3 and sums[28] >= 10000


def crafted_sums(n, xi, noise=0.0, seed=7):
    """the 29 sums of n well-spread rows J, e = J . xi + noise: map_align_main.cpp's sums_of, in numpy"""
    rng = np.random.default_rng(seed)
    J = (rng.random((n, 6)) - 0.5) * np.array([20.0] * 3 + [1.0] * 3)
    return E.np_row_sums(J, J @ np.asarray(xi, float) + noise * (rng.random(n) - 0.5))[0]


def run_loop(seq, xf, max_iter=25, min_pairs=100, eps_rot=1e-9, eps_trans=1e-9):
    """np_gauss_newton fed the sums of `seq`, one per evaluation; also the poses it asked for"""
    asked, it = [], iter(seq)

    def eval_sums(x):
        asked.append(x)
        return next(it)
    return E.np_gauss_newton(eval_sums, xf, CENTRE, max_iter, min_pairs, eps_rot, eps_trans), asked


def test_loop_verdicts_on_crafted_sums():
    """map_align_main.cpp's sequences through the yardstick's loop: the same verdicts, iteration counts and returned poses"""
    x0 = E.about(E.rotation(12.0, (1, -2, 1.5)), (3, -2, 1), CENTRE)
    xi = (0.02, 0.01, -0.03, 0.3, 0.2, -0.1)
    good, tiny = crafted_sums(500, xi), crafted_sums(500, (1e-10, -2e-10, 1e-10, 3e-10, 1e-10, -1e-10))
    for min_pairs in (0, 100):                                    # count 0
        (xf, verdict, it, sums, step), asked = run_loop([np.zeros(29)], x0, min_pairs=min_pairs)
        assert verdict == E.FEW_PAIRS and it == 0 and xf is asked[0] and not step.any()
    noisy = crafted_sums(300, xi, 0.01)                           # max_iter 0; one pair short, FEW_PAIRS comes first
    (xf, verdict, it, sums, step), asked = run_loop([noisy], x0, max_iter=0, min_pairs=300)
    assert verdict == E.ITER_LIMIT and it == 0 and xf is asked[0] and not step.any() and sums is noisy
    assert run_loop([noisy], x0, max_iter=0, min_pairs=301)[0][1] == E.FEW_PAIRS
    z = np.zeros(29)                                              # a zero matrix with enough pairs
    z[27], z[28] = 2.0, 500.0
    (xf, verdict, it, sums, step), asked = run_loop([z], x0)
    assert verdict == E.SINGULAR and it == 0 and xf is asked[0] and not step.any()
    (xf, verdict, it, sums, step), asked = run_loop([good, tiny], x0)     # one step, then a step below eps: the stepped pose, not evaluated again
    want1, s1 = E.np_step(good, CENTRE, x0)
    want2, s2 = E.np_step(tiny, CENTRE, want1)
    assert verdict == E.CONVERGED and it == 2 and len(asked) == 2 and np.array_equal(asked[1], want1) and np.array_equal(xf, want2) and np.array_equal(step, s2)
    assert np.allclose(s1, xi, rtol=0, atol=1e-12) and sums is tiny
    below = (0.9 * E.EPS_ROT_MIN, 0, 0, 0, 0.9 * E.EPS_TRANS_MIN, 0)      # the eps floor
    rot_above = (1.1 * E.EPS_ROT_MIN, 0, 0, 0, 0.9 * E.EPS_TRANS_MIN, 0)
    trans_above = (0.9 * E.EPS_ROT_MIN, 0, 0, 0, 1.1 * E.EPS_TRANS_MIN, 0)
    (xf, verdict, it, sums, step), _ = run_loop([crafted_sums(500, below)], x0, eps_rot=0.0, eps_trans=0.0)
    assert verdict == E.CONVERGED and it == 1 and 0 < step[0] < E.EPS_ROT_MIN and 0 < step[4] < E.EPS_TRANS_MIN
    for above in (rot_above, trans_above):                        # goes on: the second evaluation ends it
        (xf, verdict, it, sums, step), asked = run_loop([crafted_sums(500, above), np.zeros(29)], x0, eps_rot=0.0, eps_trans=0.0)
        assert verdict == E.FEW_PAIRS and it == 1 and len(asked) == 2
    assert run_loop([crafted_sums(500, rot_above)], x0, eps_rot=2 * E.EPS_ROT_MIN, eps_trans=0.0)[0][1] == E.CONVERGED
    few = crafted_sums(99, xi, 0.5)                               # FEW_PAIRS after one step: the pose evaluated before it
    (xf, verdict, it, sums, step), asked = run_loop([good, few], x0)
    assert verdict == E.FEW_PAIRS and it == 1 and xf is asked[0] and np.array_equal(step, s1) and sums is few and np.array_equal(asked[1], want1)
    s = x0.copy()                                                 # a start that is not rigid: the yardstick, like kf_map_refine_poses, goes on
    s[:, :3] *= 1.5
    (xf, verdict, it, sums, step), asked = run_loop([good, np.zeros(29)], s)
    assert verdict == E.FEW_PAIRS and it == 1 and len(asked) == 2


def test_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_align_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "map_align_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map align ok", out.stdout[-3000:]
