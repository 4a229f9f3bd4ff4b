"""GPU: aligning two maps.  kf_align_brick_store refines the rigid transform kf_merge_brick_store_rigid needs by Gauss-Newton on the SDF-to-SDF error
between the brick store and an incoming map; HybKinectfu::alignMap puts a map file behind it.

The yardstick is map_align_expect.py: the rule of include/hybkf.h restated in numpy (float64 for a brick's base, float32 with one rounded operation per
operation for the row, the exact products added with math.fsum), the Gauss-Newton loop over those sums, and the analytic maps: a cuboid with half extents
(14, 10, 7) voxels in a band of 4, map A the scene itself, map B the scene moved by a known X and sampled analytically, so the truth is exactly X^-1.
Everything runs at 64 voxels @ 2.0 m with a store of 1024 bricks.

The comparison of sums: n exactly; every other sum within n * 2^-52 * sum |term| of the fsum -- the first-order bound for n exact terms added in fp64 in any
order (each of the n - 1 additions errs by at most 2^-53 of a partial sum, which sum |term| bounds), doubled.  Derived, not tuned."""
import ctypes as C

import numpy as np
import pytest

import map_align_expect as E
import test_gpu_brickstore as B
import test_gpu_map_file as M
import test_gpu_map_merge as MM
import test_gpu_map_resample as R
import test_gpu_shift as G
from hybkinectfu_amd import host_app as H
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
u32 = B.u32
CAP = B.CAP
ARG, STATE = 1001, 1002
CENTRE = (32.0, 32.0, 32.0)
FAR = (500000, -400000, 300000)
EYE = np.eye(3, 4)


def device_sums(ctx, src, xf, centre):
    got, rep = ctx.align_brick_store(src[0], src[1], src[2], xf, centre, max_iter=0)
    assert rep.verdict == K.ALIGN_ITER_LIMIT and rep.iterations == 0 and np.array_equal(got, np.asarray(xf, f64))     # evaluated, xf left alone
    return np.array(rep.sums[:], f64), rep.rms


def assert_sums(ctx, dst, src, xf, centre, least, what):
    want, mags = E.np_sums(dst, src, xf, centre)
    print(what, "n", int(want[28]))
    assert want[28] >= least, what                                # numpy alone, before the library is called
    got, rms = device_sums(ctx, src, xf, centre)
    assert got[28] == want[28], (what, got[28], want[28])
    bound = want[28] * 2.0 ** -52 * mags
    worst = np.max(np.abs(got[:28] - want[:28]) / np.maximum(bound[:28], 1e-300))
    print(what, "worst |difference| / bound", worst)
    assert np.all(np.abs(got[:28] - want[:28]) <= bound[:28]), (what, got - want, bound)
    assert rms == np.sqrt(got[27] / got[28])


def points(name):
    truth = E.inverse(E.move(name))
    return (("identity", EYE), ("truth", truth), ("halfway", E.halfway(truth)))


# ---- 1. the sums against numpy; 2. the same with keys far out -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.MOVES))
def test_sums_against_numpy(name):
    a, b = E.analytic_map(), E.analytic_map(name)
    ctx = MM.store_ctx(64, False, a)
    for what, xf in points(name):
        assert_sums(ctx, a, b, xf, CENTRE, 10000, (name, what))
    ctx.close()


@pytest.mark.parametrize("name", list(E.MOVES))
def test_sums_with_keys_far_out(name):
    """both maps moved by (500000, -400000, 300000) bricks, t and centre moved along: the base corner's split into an integer and a fraction"""
    a, b = E.analytic_map(shift=FAR), E.analytic_map(name, shift=FAR)
    centre = tuple(c + 8.0 * s for c, s in zip(CENTRE, FAR))
    ctx = MM.store_ctx(64, False, a)
    for what, xf in points(name):
        assert_sums(ctx, a, b, E.moved_by_bricks(xf, FAR), centre, 10000, (name, what, "far"))
    ctx.close()


# ---- 3. real maps -----------------------------------------------------------------------------------------------------------------------------------------
SMALL = E.xf_of(E.rotation(2.0, (1, 2, 3)), (0.23, -0.17, 0.04))   # test_gpu_map_resample.GENERAL scaled down to 2 degrees and a tenth of its translation


@pytest.mark.parametrize("res,color", B.CASES)
def test_sums_on_real_maps(res, color):
    """session A in the store, session B the source: holes, bricks that only one map holds, a colour context.  numpy's n, identity / SMALL:
    see the printed counts (asserted >= 1000 before the library is called)"""
    a, b = MM.two_maps(res, color)
    lo, hi = a[0].min(axis=0), a[0].max(axis=0) + 1
    centre = tuple(4.0 * (float(l) + float(h)) for l, h in zip(lo, hi))
    ctx = MM.store_ctx(res, color, a)
    for what, xf in (("identity", EYE), ("small", SMALL)):
        assert_sums(ctx, a, b, xf, centre, 1000, (res, color, what))
    ctx.close()


# ---- 4. recovery ---------------------------------------------------------------------------------------------------------------------------------------------
_NUMPY_LOOP = {}


def numpy_loop(name):
    """the restatement's own loop from the identity, once per case: (xf, verdict, iterations, errors against the truth)"""
    if name not in _NUMPY_LOOP:
        xf, verdict, it, _, _ = E.np_align(E.analytic_map(), E.analytic_map(name), EYE, CENTRE, max_iter=25, min_pairs=1000, eps_rot=1e-9, eps_trans=1e-9)
        _NUMPY_LOOP[name] = (xf, verdict, it, E.errors(xf, E.inverse(E.move(name)), CENTRE))
    return _NUMPY_LOOP[name]


@pytest.mark.parametrize("name", list(E.MOVES))
def test_recovery(name):
    """From the identity, max_iter 25, eps 1e-9, centre (32, 32, 32).  Errors against X^-1 as (distance of the images of the centre in voxels, angle in
    radians), numpy's loop / the device's, which may be at most twice numpy's:
      2deg:   numpy (0.005649819433797, 1.5112123066956e-4) in 5 steps   device (0.005649819433805, 1.5112123066952e-4) in 5 steps
      5deg:   numpy (0.001276840150847, 2.8389074321291e-4) in 5 steps   device (0.001276840150840, 2.8389074321298e-4) in 5 steps
      10deg:  numpy (0.000884414519940, 1.6470587344423e-4) in 6 steps   device (0.000884414519937, 1.6470587344421e-4) in 6 steps
    (measured on an MI355X; both sets are printed by the test).
    An eps of 1e-9 lies below what the fp32 rule resolves: the restatement's steps stay near 3e-9 rad and 2e-8 voxels for ever (an fp64 rule would reach
    1e-13), so the library raises an eps to KF_ALIGN_EPS_ROT_MIN / KF_ALIGN_EPS_TRANS_MIN, and so does the restatement's loop."""
    a, b = E.analytic_map(), E.analytic_map(name)
    truth = E.inverse(E.move(name))
    _, nv, nit, nerr = numpy_loop(name)
    print(name, "numpy: verdict", nv, "iterations", nit, "errors", nerr)
    assert nv == E.CONVERGED
    ctx = MM.store_ctx(64, False, a)
    xf, rep = ctx.align_brick_store(b[0], b[1], b[2], EYE, CENTRE, max_iter=25, min_pairs=1000, eps_rot=1e-9, eps_trans=1e-9)
    ctx.close()
    err = E.errors(xf, truth, CENTRE)
    print(name, "device: verdict", rep.verdict, "iterations", rep.iterations, "errors", err, "rms", rep.rms, "pairs", rep.sums[28])
    assert rep.verdict == K.ALIGN_CONVERGED
    assert err[0] <= 2 * nerr[0] and err[1] <= 2 * nerr[1]


# ---- 5. reproducible ----------------------------------------------------------------------------------------------------------------------------------------------
def test_reproducible():
    a, b = E.analytic_map(), E.analytic_map("5deg")
    runs = []
    for _ in range(2):                                            # two contexts loaded in the same write order, two calls each
        ctx = MM.store_ctx(64, False, a)
        for _ in range(2):
            s0 = device_sums(ctx, b, E.halfway(E.inverse(E.move("5deg"))), CENTRE)[0]
            xf, rep = ctx.align_brick_store(b[0], b[1], b[2], EYE, CENTRE)
            runs.append(s0.tobytes() + xf.tobytes() + bytes(rep))
        ctx.close()
    assert runs[1] == runs[0] and runs[3] == runs[2]              # the same call twice
    assert runs[2] == runs[0]                                     # a second context


# ---- 6. bystander ---------------------------------------------------------------------------------------------------------------------------------------------------
def digest(ctx, color):
    store = ctx.brick_store()                                     # in slot order
    maps = [ctx.download_map(m).tobytes() for m in (K.MAP_MODEL_VERTICES, K.MAP_MODEL_NORMALS)]
    planes = M.planes_bits(ctx, color)
    return ([x.tobytes() for x in store if x is not None], ctx.brick_store_count(), [x.tobytes() for x in planes if x is not None], G.pose_of(ctx).tobytes(),
            ctx.volume_origin(), maps, ctx.triangles().tobytes())


def test_bystanders_are_untouched():
    res, color = 64, False
    _, b = MM.two_maps(res, color)
    ctx, twin = MM.session(res, color, "A"), MM.session(res, color, "A")
    for c in (ctx, twin):
        c.brick_store_capture()
        G.raycast(c, color)
        c.marching_cubes(300 * c.size / res)
    before = digest(ctx, color)
    assert len(before[6]) > 0 and before[1][0] > 0
    lo, hi = ctx.brick_store_bounds()
    xf, rep = ctx.align_brick_store(b[0], b[1], b[2], SMALL, tuple(4.0 * (l + h) for l, h in zip(lo, hi)))
    print("bystander: verdict", rep.verdict, "iterations", rep.iterations, "pairs", rep.sums[28])
    assert rep.iterations >= 1 and not np.array_equal(xf, SMALL)   # a full alignment ran
    assert digest(ctx, color) == before
    oka, pa = G.run_frame(ctx, 6)                                 # and the next frame is a twin's
    okb, pb = G.run_frame(twin, 6)
    assert oka == okb and np.array_equal(u32(pa), u32(pb)) and M.same_planes(ctx, twin)
    ctx.close(); twin.close()


# ---- 7. verdicts and refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_verdicts():
    a = E.analytic_map()
    ctx = MM.store_ctx(64, False, a)
    away = E.analytic_map("2deg", shift=(40, 0, 0))               # a source that overlaps nothing
    xf, rep = ctx.align_brick_store(away[0], away[1], away[2], EYE, CENTRE)
    assert rep.verdict == K.ALIGN_FEW_PAIRS and rep.iterations == 0 and np.array_equal(xf, EYE) and rep.sums[28] == 0 and rep.rms == 0
    xf, rep = ctx.align_brick_store(away[0][:0], away[1][:0], away[2][:0], EYE, CENTRE)      # no source at all
    assert rep.verdict == K.ALIGN_FEW_PAIRS and np.array_equal(xf, EYE)
    ctx.close()
    # two parallel planes only, the source the same planes moved without a turn: the two translations along the planes and the turn about their normal are
    # free.  With R = I their columns of J are exact zeros (every corner value depends on z alone), so the third pivot is exactly 0
    sa, sb = E.slab_maps()
    ctx = MM.store_ctx(64, False, sa)
    for guess in (EYE, E.xf_of(np.eye(3), (0.3, -0.2, 0.4))):
        xf, rep = ctx.align_brick_store(sb[0], sb[1], sb[2], guess, CENTRE)
        print("slab: verdict", rep.verdict, "iterations", rep.iterations, "pairs", rep.sums[28])
        assert rep.sums[28] >= 1000 and rep.verdict in (K.ALIGN_SINGULAR, K.ALIGN_ITER_LIMIT) and np.array_equal(xf, guess)
        assert np.all(np.isfinite(xf)) and np.all(np.isfinite(np.array(rep.sums[:]))) and np.all(np.isfinite(np.array(rep.step[:])))
    # a tilted guess: the free unknowns' pivots are rounding noise of either sign, the verdict whatever follows from that, but never a NaN
    xf, rep = ctx.align_brick_store(sb[0], sb[1], sb[2], E.xf_of(E.rotation(1.0, (1, 2, 3)), (0.2, 0.1, -0.3)), CENTRE)
    print("slab, tilted guess: verdict", rep.verdict, "iterations", rep.iterations, "pairs", rep.sums[28])
    assert np.all(np.isfinite(xf)) and np.all(np.isfinite(np.array(rep.sums[:]))) and np.all(np.isfinite(np.array(rep.step[:])))
    ctx.close()


def align_raw(ctx, n, keys, t, w, xf, params, report):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return K.load().kf_align_brick_store(ctx.h if ctx is not None else None, n, p(keys), p(t), p(w), xf, C.byref(params) if params is not None else None,
                                        C.byref(report) if report is not None else None)


def test_refusals_touch_nothing():
    a, b = E.analytic_map(), E.analytic_map("2deg")
    ctx = MM.store_ctx(64, False, a)
    before = (M.planes_bits(ctx), [x.tobytes() for x in ctx.brick_store() if x is not None], ctx.brick_store_count())
    k2, t2, w2 = np.ascontiguousarray(b[0][:2]), np.ascontiguousarray(b[1][:2]), np.ascontiguousarray(b[2][:2])
    guess = E.xf_of(E.rotation(1.0, (1, 2, 3)), (0.2, 0.1, -0.3))
    good = lambda: K.align_params(CENTRE)
    tried = []

    def refused(code, keys=k2, t=t2, w=w2, xf=guess, params="good", report="yes"):
        x = K.rigid_xf(xf) if xf is not None else None
        rep = K.AlignReport() if report else None
        raw = bytes(rep) if rep is not None else b""
        got = align_raw(ctx, 2, keys, t, w, x, good() if params == "good" else params, rep)
        tried.append(got)
        return got == code and (x is None or bytes(x) == np.asarray(xf, f64).tobytes()) and (rep is None or bytes(rep) == raw)

    assert refused(ARG, keys=None) and refused(ARG, t=None) and refused(ARG, w=None) and refused(ARG, xf=None)
    assert refused(ARG, params=None) and refused(ARG, report=None)
    scaled, mirror, nan = guess.copy(), guess.copy(), guess.copy()
    scaled[:, :3] *= 1.001; mirror[0, :3] *= -1; nan[1, 3] = np.nan
    for bad in (scaled, mirror, nan):                             # no rigid transform
        assert refused(ARG, xf=bad)
    assert refused(ARG, keys=np.ascontiguousarray(np.stack([b[0][0], b[0][0]])))                               # a key twice
    assert refused(ARG, keys=np.ascontiguousarray(np.stack([b[0][0], np.array((1 << 20, 0, 0), np.int32)])))   # a key out of range
    for field, value in (("eps_rot", np.nan), ("eps_trans", np.inf), ("eps_rot", -1.0)):
        p = good()
        setattr(p, field, value)
        assert refused(ARG, params=p), field
    p = good()
    p.centre[1] = np.nan
    assert refused(ARG, params=p)
    assert len(tried) == 15
    after = (M.planes_bits(ctx), [x.tobytes() for x in ctx.brick_store() if x is not None], ctx.brick_store_count())
    assert M.equal_bits(after[0], before[0]) and after[1:] == before[1:]
    assert align_raw(None, 2, k2, t2, w2, K.rigid_xf(guess), good(), K.AlignReport()) == ARG
    ctx.close()
    bare = G.make_ctx(64)                                         # no store
    assert align_raw(bare, 2, k2, t2, w2, K.rigid_xf(guess), good(), K.AlignReport()) == STATE and bare.brick_store_count() == (0, 0, 0)
    bare.close()
    slab = G.make_ctx(64, slab=(0, 32), halo=8)                   # a z-slab context
    assert align_raw(slab, 2, k2, t2, w2, K.rigid_xf(guess), good(), K.AlignReport()) == ARG
    slab.close()


def test_slab_application_refuses(tmp_path):
    sl = H.SlabsApp(64, 2.0, G.CAM, [0, 32, 64])
    try:
        ok, found, rep = sl.align_map(str(tmp_path / "x.hkfmap"), np.eye(4, dtype=f32))
        assert ok is False and np.array_equal(found, np.eye(4, dtype=f32)) and rep is None
    finally:
        sl.close()


# ---- 8. the host class ---------------------------------------------------------------------------------------------------------------------------------------------------
def app_with_map(m, path):
    """an application whose store holds the analytic map m, saved to `path` through saveMap (the window is empty: the capture adds nothing)"""
    app = M.make_app(64, 2.0, G.CAM, False)
    try:
        app.set_brick_store(CAP)
        ctx = K.Context.borrow(app.ctx_handle(), K.camera(*G.CAM), 64, 2.0)
        ctx.write_brick_store(m[0], m[1], m[2], None)
        assert app.save_map(path)
    except Exception:
        app.close()
        raise
    return app, ctx


def test_host_class_aligns_then_merges(tmp_path):
    """App.align_map from the identity against the 5deg map: test 4's bar, in metres.  Then merge_map_rigid with the matrix found gives the store that
    np_resample + np_merge give for that matrix, bit for bit: the two features compose."""
    name = "5deg"
    a, b = E.analytic_map(), E.analytic_map(name)
    fa, fb = str(tmp_path / "a.hkfmap"), str(tmp_path / "b.hkfmap")
    app, _ = app_with_map(b, fb)
    app.close()
    app, ctx = app_with_map(a, fa)
    try:
        held = B.store_sorted(ctx)
        assert M.same_store(held, a)
        mb = MM.records(fb, False)[0]
        ok, found, rep = app.align_map(fb, np.eye(4, dtype=f32))
        cell = f32(2.0) / f32(64)
        # the centre the class uses: the middle of the store's box
        lo, hi = a[0].min(axis=0), a[0].max(axis=0) + 1
        centre = np.array([4.0 * (float(l) + float(h)) for l, h in zip(lo, hi)])
        truth = E.inverse(E.move(name))
        xf = E.xf_of(found[:3, :3].astype(f64), found[:3, 3].astype(f64) / f64(cell))      # in voxels, as the class hands it to the merge
        err = E.errors(xf, truth, CENTRE)
        nerr = numpy_loop(name)[3]
        print("host class: verdict", rep.verdict, "iterations", rep.iterations, "errors", err, "numpy", nerr, "centre", centre)
        assert ok and rep.verdict == K.ALIGN_CONVERGED
        assert err[0] * float(cell) <= 2 * nerr[0] * float(cell) and err[1] <= 2 * nerr[1]
        assert M.same_store(B.store_sorted(ctx), held)            # nothing merged
        assert app.merge_map_rigid(fb, found)
        want = MM.np_merge(a, R.observed(R.np_resample(mb, xf)[0]))
        got = B.store_sorted(ctx)
        assert len(want[0]) >= len(a[0]) and M.same_store(got, want)
    finally:
        app.close()
