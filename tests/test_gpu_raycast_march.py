"""GPU: the instantiated march trip and the tile prologue against the ORACLE, bit for bit, at the smallest shapes where each of their paths first exists.

rc_march (csrc/raycast_tile.h) compiles its loop once per way of forming `pos * res / size` -- the quotient, two multiplications (size 2^n), one
multiplication (size and resolution 2^n, res >= size) -- clamps with a median of three and walks two additions per round.  raycast_scenarios.py
already reaches the quotient at 104^3 and 64^3 @ 3 m and the one multiplication at 128^3 @ 4 m; here:
  96^3 @ 4 m     size 2^n, resolution not: two multiplications; 12 bricks, 3 macro and 6 meso cells per axis
  64^3 @ 128 m   both 2^n but res < size: the one-multiplication form's guard (it must NOT be taken)
  256^3 @ 4 m    the tile bounds' direct scan over 16 meso cells per row, and (KF_RAYCAST_BOUNDS_MESO=0) over 8 macro cells = one byte per row; each
                 also without bounds (KF_RAYCAST_BOUNDS=0): the same maps
  128^3 as two z-slabs  lanes outside the stored layers (the second slab's bz0 > 0); merged maps == whole-volume maps
  128^3 with KF_RAYCAST_NEG_LDS=0 / KF_RAYCAST_MESO=0  the conditional flag read / the absent meso lookup
Vertices, normals and pyramid levels 1-2 are compared.  One child process per switch set (raycast_march_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_march_cases as M
import raycast_scenarios as R
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORM_FIELDS = [name for name, _ in K.RaycastForm._fields_]
TAGS = ("v", "n", "v1", "v2", "n1", "n2")
_ABORT = []                 # a child that died or hung: no further child is started


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """the analytic volumes written for the children, and the oracle's maps of every call (computed once)"""
    voldir = tmp_path_factory.mktemp("march_volumes")
    maps = {}
    for vid in M.VOLUME_IDS:
        case = M.CASES[vid]
        data = R.analytic_volume(case[1], case[2])
        np.save(str(voldir / (vid + "_tsdf.npy")), data[0])
        np.save(str(voldir / (vid + "_weight.npy")), data[1])
        cases = [case] + ([M.SLAB_CASE] if vid == M.SLAB_CASE[0] else [])
        vol, _ = M.as_scenario(case)
        ovol = R.oracle_volume(vol, data)
        del data
        for c in cases:
            for call in M.as_scenario(c)[1]:
                if call[0] not in maps:
                    maps[call[0]] = R.oracle_maps(vol, ovol, call)
        del ovol
    return dict(voldir=str(voldir), maps=maps)


def _cast(oracle, tmp_path, env, cases):
    assert not _ABORT, "not started: " + _ABORT[0]
    e = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k in ("KF_STATS_CROSSCHECK", "KF_ORACLE_SO", "KF_LIB")}
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    out = str(tmp_path / ("out_%d.npz" % len(os.listdir(str(tmp_path)))))
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "raycast_march_child.py"), out, oracle["voldir"]] + list(cases), env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _ABORT.append("the child of %s %s timed out" % (env, cases))
        pytest.fail(_ABORT[0])
    if r.returncode != 0:
        _ABORT.append("the child of %s %s exited with %d" % (env, cases, r.returncode))
        pytest.fail(_ABORT[0] + "\n" + r.stderr[-3000:])
    got = dict(np.load(out))
    os.remove(out)
    return got


def _form(got, k):
    return dict(zip(FORM_FIELDS, (int(x) for x in got[M.key(k) + "_form"])))


def _against_oracle(got, oracle, case, prefix=""):
    bad = []
    for k, name, _, _, _ in M.calls(case):
        want = oracle["maps"][k]
        for tag in TAGS:
            g = got.get(prefix + M.key(k) + "_" + tag)
            if g is None:
                continue
            if not np.array_equal(g, want[tag].view(np.uint32)):
                diff = (g != want[tag].view(np.uint32)).any(axis=-1)
                bad.append("%s %s: %d pixels differ, first at %s" % (k, tag, int(diff.sum()), tuple(int(i) for i in np.argwhere(diff)[0])))
    assert not bad, (bad[:20], len(bad))


def test_cases_state_their_hits(oracle):
    """no case passes on nothing: every view has its hits on the oracle's side, the grazing view on a tenth of its pixels, `away` on none"""
    for case in list(M.CASES.values()) + [M.SLAB_CASE]:
        cam = case[3]
        for k, name, _, _, _ in M.calls(case):
            h = R.hits(oracle["maps"][k]["n"])
            assert h >= R.min_hits(name, cam) and (h == 0) == (name in R.ZERO_HIT_VIEWS), (k, h)
            if name == "graze-y":
                assert 10 * h >= cam[0] * cam[1], (k, h)


@pytest.mark.parametrize("cid", ["m96", "m64"])
def test_scaling_forms_equal_the_oracle(cid, oracle, tmp_path):
    case = M.CASES[cid]
    got = _cast(oracle, tmp_path, {}, [cid])
    for k, _, _, _, _ in M.calls(case):
        f = _form(got, k)
        assert f["tile_bounds"] == 1 and f["bounds_path"] == K.RC_BOUNDS_MESO and f["meso_lds"] == 1 and f["neg_lds"] == 1, (k, f)
    _against_oracle(got, oracle, case)


@pytest.mark.parametrize("bounds_meso,path", [(None, K.RC_BOUNDS_MESO), ("0", K.RC_BOUNDS_MACRO)], ids=["meso-rows-of-two-bytes", "macro-rows-of-one-byte"])
def test_direct_scan_bounds_equal_the_oracle_and_no_bounds(bounds_meso, path, oracle, tmp_path):
    case = M.CASES["m256"]
    env = {} if bounds_meso is None else {"KF_RAYCAST_BOUNDS_MESO": bounds_meso}
    bounded = _cast(oracle, tmp_path, env, ["m256"])
    for k, _, _, _, _ in M.calls(case):
        f = _form(bounded, k)
        assert f["tile_bounds"] == 1 and f["bounds_path"] == path, (k, f)
    _against_oracle(bounded, oracle, case)
    free = _cast(oracle, tmp_path, dict(env, KF_RAYCAST_BOUNDS="0"), ["m256"])
    for k, _, _, _, _ in M.calls(case):
        f = _form(free, k)
        assert f["tile_bounds"] == 0 and f["bounds_path"] == K.RC_BOUNDS_NONE, (k, f)
        for tag in TAGS:
            assert np.array_equal(free[M.key(k) + "_" + tag], bounded[M.key(k) + "_" + tag]), (k, tag)
    _against_oracle(free, oracle, case)


def test_two_z_slabs_equal_the_whole_volume(oracle, tmp_path):
    got = _cast(oracle, tmp_path, {}, ["slabs"])
    stored = got["slabs_stored"]
    assert stored[1][0] > 0 and stored[1][0] < M.SLAB_RANGES[1][0] and stored[0][1] > M.SLAB_RANGES[0][1], stored      # owned inside stored; second slab's bz0 > 0
    _against_oracle(got, oracle, M.SLAB_CASE)                 # the whole volume
    for k, _, _, _, _ in M.calls(M.SLAB_CASE):
        assert int(got["slabs_" + M.key(k) + "_owners"].max()) == 1, k
        for tag in ("v", "n"):
            assert np.array_equal(got["slabs_" + M.key(k) + "_" + tag], got[M.key(k) + "_" + tag]), (k, tag)


@pytest.mark.parametrize("switch,field", [("KF_RAYCAST_NEG_LDS", "neg_lds"), ("KF_RAYCAST_MESO", "meso_lds")])
def test_table_switches_equal_the_oracle(switch, field, oracle, tmp_path):
    case = M.CASES["m128"]
    got = _cast(oracle, tmp_path, {switch: "0"}, ["m128"])
    for k, _, _, _, _ in M.calls(case):
        f = _form(got, k)
        assert f[field] == 0 and f["tile_bounds"] == 1, (k, f)
    _against_oracle(got, oracle, case)
