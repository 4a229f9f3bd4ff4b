"""GPU: the raycast's switchable forms give the same bits.

The crossing's gradient (gradientForPoint, src/cuda/raycastingVolume.cu:16-42) is evaluated from one shared 32-voxel neighbourhood
(csrc/grad_shared.h) with a wave-level fallback to six separate lookups for taps whose cell is not "the vertex's cell moved by one".  Real data never
takes the fallback, so KF_RAYCAST_SHARED_GRAD=2 sends every other wave down it; 0 switches the shared form off.  The maps of all three -- whole
volume (k_raycast) and a stored z-slab (k_slab_ray_normals) -- and of the launches without tile bounds / meso table must be identical.  That the
default form equals the ORACLE bit for bit is test_gpu_parity.py's business (same process, default switches).

Below the digest test: every switch set against the ORACLE, from every side (raycast_forms_child.py, raycast_scenarios.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_scenarios as R
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _digest(env_extra, res, cols, rows):
    env = dict(os.environ)
    for k in ("KF_RAYCAST_SHARED_GRAD", "KF_RAYCAST_VIEW_HALF", "KF_RAYCAST_BOUNDS", "KF_RAYCAST_MESO"):
        env.pop(k, None)
    env.update(env_extra)
    env["PYTHONPATH"] = os.path.dirname(HERE) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(HERE, "raycast_digest.py"), str(res), str(cols), str(rows)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("res,cols,rows", [(128, 320, 240), (96, 200, 150)])
def test_gradient_forms_and_table_switches_give_the_same_maps(res, cols, rows):
    ref = _digest({}, res, cols, rows)
    assert ref["whole0hits"] > cols * rows // 3 and ref["whole1hits"] > cols * rows // 3 and ref["slab0hits"] > 200       # there is something to compare
    # (KF_RAYCAST_VIEW_HALF: the gathers' raw-buffer view reaches that many brick layers to either side of the wave's first lane instead of 2 GB worth --
    # a small volume then meets what 1024^3 / 2048^3 meet: views that start inside the volume, waves whose lanes do not fit one view)
    for env in ({"KF_RAYCAST_SHARED_GRAD": "0"}, {"KF_RAYCAST_SHARED_GRAD": "2"}, {"KF_RAYCAST_VIEW_HALF": "1"}, {"KF_RAYCAST_VIEW_HALF": "3"},
                {"KF_RAYCAST_BOUNDS": "0", "KF_RAYCAST_MESO": "0"}):
        assert _digest(env, res, cols, rows) == ref, env


# ---- every switchable form against the ORACLE, from every side (raycast_forms_child.py, raycast_scenarios.py) -------------------------------------
# The raycast's skipping (super / macro / meso / brick tables, the per-tile frustum bounds of rc_tile_bounds on three paths, the sign-dependent cell walk,
# the closed-form advance to the tile bound) must be conservative from any viewpoint.  A child process per switch set casts every scenario -- analytic
# volumes at 104^3 (partial macro and meso cells), 128^3 @ 4 m (the power-of-two voxel path), 384^3 (the direct macro scan), 64^3 with colour, and a
# volume fused from three sides -- from ~25 viewpoints; the parent compares every map with the oracle bit for bit, checks each call's form against a
# model of the dispatcher (kf_get_raycast_form) and at the end that every form listed in ALL_FORMS ran.
ROOT = os.path.dirname(HERE)
FORM_FIELDS = [name for name, _ in K.RaycastForm._fields_]
RC_SWITCHES = ("KF_RAYCAST_SHARED_GRAD", "KF_RAYCAST_VIEW_HALF", "KF_RAYCAST_BOUNDS", "KF_RAYCAST_BOUNDS_MESO", "KF_RAYCAST_MESO", "KF_RAYCAST_NEG_LDS",
               "KF_RAYCAST_PYRAMID")
SETS = [
    ("default", {}),
    ("shared-grad0", {"KF_RAYCAST_SHARED_GRAD": "0"}),
    ("shared-grad2", {"KF_RAYCAST_SHARED_GRAD": "2"}),
    ("view-half1", {"KF_RAYCAST_VIEW_HALF": "1"}),
    ("view-half3", {"KF_RAYCAST_VIEW_HALF": "3"}),
    ("bounds0", {"KF_RAYCAST_BOUNDS": "0"}),
    ("bounds2", {"KF_RAYCAST_BOUNDS": "2"}),
    ("bounds-meso0", {"KF_RAYCAST_BOUNDS_MESO": "0"}),
    ("meso0", {"KF_RAYCAST_MESO": "0"}),
    ("bounds2-meso0", {"KF_RAYCAST_BOUNDS": "2", "KF_RAYCAST_MESO": "0"}),
    ("neg-lds0", {"KF_RAYCAST_NEG_LDS": "0"}),
    ("pyramid0", {"KF_RAYCAST_PYRAMID": "0"}),
]
BOUNDS_NAMES = {K.RC_BOUNDS_NONE: "none", K.RC_BOUNDS_MESO: "meso", K.RC_BOUNDS_MACRO: "macro", K.RC_BOUNDS_LIST: "list"}
# every form of the launch this test reaches: the tile-bounds path, where the tables live, the gradient's mode and view, the in-launch pyramid
ALL_FORMS = {"bounds:none", "bounds:meso", "bounds:macro", "bounds:list", "bounds:list+meso_lds0", "meso_lds:0", "meso_lds:1", "neg_lds:0", "neg_lds:1",
             "grad:0", "grad:1", "grad:2", "view_half:0", "view_half:1", "view_half:3", "pyramid:0", "pyramid:1"}


def form_names(f):
    b = BOUNDS_NAMES[f["bounds_path"]]
    out = {"bounds:" + b, "meso_lds:%d" % f["meso_lds"], "neg_lds:%d" % f["neg_lds"], "grad:%d" % f["shared_grad"], "view_half:%d" % f["view_half"],
           "pyramid:%d" % f["pyramid"]}
    if b == "list" and not f["meso_lds"]:
        out.add("bounds:list+meso_lds0")
    return out


class Model:
    """raycast_launch's choice (raycast.hip), written out again from its documentation: the form of a k_raycast call into the model maps under a
    switch set, for a volume of `res` voxels per axis at the stock pyramid depth"""

    def __init__(self, env):
        g = lambda k, d: int(env[k]) if k in env else d        # noqa: E731  (atoi of the variable, or the default)
        mode, half = g("KF_RAYCAST_SHARED_GRAD", 1), g("KF_RAYCAST_VIEW_HALF", 0)
        self.grad = 0 if mode <= 0 else mode & 255
        self.half = 0 if mode <= 0 or not 0 < half < 4096 else half
        self.bounds = g("KF_RAYCAST_BOUNDS", 1)
        self.bounds_meso = g("KF_RAYCAST_BOUNDS_MESO", 1)
        self.meso = g("KF_RAYCAST_MESO", 1)
        self.neg = g("KF_RAYCAST_NEG_LDS", 1)
        self.pyr = g("KF_RAYCAST_PYRAMID", 1)

    def form(self, res, cam, call_no):
        nb = res // 8
        nm, nq = -(-nb // 4), -(-nb // 2)
        meso_lds = int(self.meso != 0)                          # (the tables of every volume here fit into the LDS budget)
        if not self.bounds:
            path = K.RC_BOUNDS_NONE
        elif self.bounds != 2 and self.bounds_meso and meso_lds and nq ** 3 <= 8192:
            path = K.RC_BOUNDS_MESO
        elif self.bounds != 2 and nm ** 3 <= 8192:
            path = K.RC_BOUNDS_MACRO
        else:
            path = K.RC_BOUNDS_LIST
        return dict(kernel=K.RC_PLAIN, fast=0, output=K.RC_OUT_MAPS, tile_bounds=int(self.bounds != 0), bounds_path=path, meso_lds=meso_lds,
                    neg_lds=int(self.neg != 0), shared_grad=self.grad, view_half=self.half, pyramid=int(self.pyr != 0),
                    grid=-(-cam[0] // 32) * -(-cam[1] // 16), calls=call_no)


@pytest.fixture(scope="module")
def rc_oracle(tmp_path_factory):
    """the analytic volumes written for the children, and the oracle's maps of every call"""
    voldir = tmp_path_factory.mktemp("raycast_volumes")
    maps, planes = {}, None
    for vol in R.VOLUMES:
        data = R.volume_data(vol)
        if vol[0] == "fused":
            planes = (data[0].view(np.uint32).copy(), data[1].view(np.uint32).copy())
        else:
            np.save(str(voldir / (vol[0] + "_tsdf.npy")), data[0])
            np.save(str(voldir / (vol[0] + "_weight.npy")), data[1])
            if data[2] is not None:
                np.save(str(voldir / (vol[0] + "_rgb.npy")), data[2])
        ovol = R.oracle_volume(vol, data)
        del data
        for call in R.calls(vol):
            maps[call[0]] = R.oracle_maps(vol, ovol, call)
        del ovol
    return dict(voldir=str(voldir), maps=maps, planes=planes)


_RC_ABORT = []              # a child that died, hung or failed: no further child is started
_RC_SEEN = {"forms": set(), "sets": set(), "started": set()}


def _rc_child_env(env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k in ("KF_STATS_CROSSCHECK", "KF_ORACLE_SO", "KF_LIB")}
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    return e


def test_scenarios_state_their_hits(rc_oracle):
    """every scenario has something to compare (or, looking away / from behind every surface, exactly nothing) -- on the oracle's side"""
    for vol in R.VOLUMES:
        for k, cam, view, _, _, _ in R.calls(vol):
            h = R.hits(rc_oracle["maps"][k]["n"])
            assert h >= R.min_hits(view, cam) and (h == 0) == (view in R.ZERO_HIT_VIEWS), (k, h)
            if view not in R.ZERO_HIT_VIEWS and vol[3]:
                assert int(np.count_nonzero(rc_oracle["maps"][k]["rgb"])) > 3 * R.min_hits(view, cam), k


@pytest.mark.parametrize("sid,env", SETS, ids=[s[0] for s in SETS])
def test_raycast_form_equals_the_oracle(sid, env, rc_oracle, tmp_path):
    if _RC_ABORT:
        pytest.skip("not started: " + _RC_ABORT[0])
    assert all(k in RC_SWITCHES for k in env), env
    _RC_SEEN["started"].add(sid)
    out = str(tmp_path / "out.npz")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "raycast_forms_child.py"), out, rc_oracle["voldir"]], env=_rc_child_env(env), cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _RC_ABORT.append("the child of %s timed out" % sid)
        pytest.fail(_RC_ABORT[0])
    if r.returncode != 0:
        _RC_ABORT.append("the child of %s exited with %d" % (sid, r.returncode))
        pytest.fail(_RC_ABORT[0] + "\n" + r.stderr[-3000:])
    got = np.load(out)
    model = Model(env)
    # the fusion pass's planes first: the flags it maintains are what the fused scenarios test
    assert np.array_equal(got["fused_tsdf"], rc_oracle["planes"][0]) and np.array_equal(got["fused_weight"], rc_oracle["planes"][1]), sid
    bad = []
    for vol in R.VOLUMES:
        n_call = {}
        for k, cam, view, _, _, _ in R.calls(vol):
            kk = k.replace("/", "__")
            want = rc_oracle["maps"][k]
            n_call[cam] = n_call.get(cam, 0) + 1
            f = dict(zip(FORM_FIELDS, (int(x) for x in got[kk + "_form"])))
            assert f == model.form(vol[1], cam, n_call[cam]), (sid, k, f, model.form(vol[1], cam, n_call[cam]))
            _RC_SEEN["forms"] |= form_names(f)
            for tag in ("v", "n", "v1", "v2", "n1", "n2"):
                if not np.array_equal(got[kk + "_" + tag], want[tag].view(np.uint32)):
                    diff = (got[kk + "_" + tag] != want[tag].view(np.uint32)).any(axis=-1)
                    bad.append("%s %s: %d pixels differ, first at %s" % (k, tag, int(diff.sum()), tuple(int(i) for i in np.argwhere(diff)[0])))
            if want["rgb"] is not None and not np.array_equal(got[kk + "_rgb"], want["rgb"]):
                bad.append("%s rgb" % k)
    os.remove(out)
    assert not bad, (sid, bad[:20], len(bad))
    _RC_SEEN["sets"].add(sid)


def test_every_raycast_form_ran():
    if _RC_ABORT:
        pytest.skip("not started: " + _RC_ABORT[0])
    if not _RC_SEEN["started"]:
        pytest.skip("no switch set ran in this session (deselected)")
    assert _RC_SEEN["sets"] == {s[0] for s in SETS}, "a switch set failed: " + str(sorted({s[0] for s in SETS} - _RC_SEEN["sets"]))
    assert _RC_SEEN["forms"] == ALL_FORMS, (sorted(ALL_FORMS - _RC_SEEN["forms"]), sorted(_RC_SEEN["forms"] - ALL_FORMS))
