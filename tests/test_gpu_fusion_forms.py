"""GPU: every form of the fusion pass against the CPU oracle, bit for bit.

kf_integrate_volume picks one of ~20 instantiations of the fusion kernel and one of four culls per call, from environment switches read once per
process (KF_INTEGRATE_BR / _PIPE / _PAIRS / _COLOR_PAIRS / _GRID / _SAT / _FREESPACE, KF_CULL_SIFT / _FINE / _MACRO_DEPTH, KF_OBSERVED_COUNT,
KF_CULL_IN_TRACK), the volume's size and the context's state.  The rest of the suite runs in one process with the defaults and reaches a handful of
them.  Here a child process (fusion_forms_child.py) fuses the scenarios of fusion_scenarios.py under one switch set each -- a queue that is no multiple
of the bricks in flight, grids smaller than the queue, partial macro cells, a slab with bz0 != 0, pending deferred weights meeting a kernel that does
not defer, colour, the device-resident pose with the tail cull -- and the parent compares planes, colour, per-frame update counts and observed-voxel
counts with the oracle's, checks that every frame ran the form its switch set selects (kf_get_fusion_form), and at the end that every form the
dispatcher can launch in the product build has run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_scenarios as F
from hybkinectfu_amd import lib as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORM_FIELDS = [name for name, _ in K.FusionForm._fields_]

# the switches kf_integrate_volume, kf_get_volume_stats and kf_icp_track read (a name outside this list is a typo in a switch set)
SWITCHES = ("KF_INTEGRATE_BR", "KF_INTEGRATE_PIPE", "KF_INTEGRATE_PAIRS", "KF_INTEGRATE_COLOR_PAIRS", "KF_INTEGRATE_GRID", "KF_INTEGRATE_SAT",
            "KF_INTEGRATE_FREESPACE", "KF_CULL_SIFT", "KF_CULL_FINE", "KF_CULL_MACRO_DEPTH", "KF_OBSERVED_COUNT", "KF_CULL_IN_TRACK")
# (id, environment, child options)
SETS = [
    ("default", {}, []),
    ("default-ask-every", {}, ["--ask", "every"]),
    ("br1-pipe0", {"KF_INTEGRATE_BR": "1", "KF_INTEGRATE_PIPE": "0"}, []),
    ("br2-pipe0", {"KF_INTEGRATE_BR": "2", "KF_INTEGRATE_PIPE": "0"}, []),
    ("br4-pipe0", {"KF_INTEGRATE_BR": "4", "KF_INTEGRATE_PIPE": "0"}, []),
    ("pipe1", {"KF_INTEGRATE_PIPE": "1"}, []),
    ("pairs0-br1", {"KF_INTEGRATE_PAIRS": "0", "KF_INTEGRATE_BR": "1"}, []),
    ("pairs0-br2", {"KF_INTEGRATE_PAIRS": "0", "KF_INTEGRATE_BR": "2"}, []),
    ("pairs0-br4", {"KF_INTEGRATE_PAIRS": "0", "KF_INTEGRATE_BR": "4"}, []),
    ("color-pairs0", {"KF_INTEGRATE_COLOR_PAIRS": "0"}, []),
    ("count1-br1-pipe0", {"KF_OBSERVED_COUNT": "1", "KF_INTEGRATE_BR": "1", "KF_INTEGRATE_PIPE": "0"}, ["--ask", "every"]),
    ("count1-br4", {"KF_OBSERVED_COUNT": "1", "KF_INTEGRATE_BR": "4"}, ["--ask", "every"]),
    ("count1-pipe1", {"KF_OBSERVED_COUNT": "1", "KF_INTEGRATE_PIPE": "1"}, ["--ask", "every"]),
    ("cull-sift1", {"KF_CULL_SIFT": "1"}, []),
    ("cull-fine0", {"KF_CULL_FINE": "0"}, []),
    ("cull-fine1", {"KF_CULL_FINE": "1"}, []),
    ("cull-macro-depth0", {"KF_CULL_MACRO_DEPTH": "0"}, []),
    ("grid64-br4", {"KF_INTEGRATE_GRID": "64", "KF_INTEGRATE_BR": "4"}, []),
    ("grid97-pipe1", {"KF_INTEGRATE_GRID": "97", "KF_INTEGRATE_PIPE": "1"}, []),
    ("freespace0", {"KF_INTEGRATE_FREESPACE": "0"}, []),
    ("sat2", {"KF_INTEGRATE_SAT": "2"}, ["--no-set-defer"]),
    ("sat0", {"KF_INTEGRATE_SAT": "0"}, ["--no-set-defer"]),
    ("cull-in-track0", {"KF_CULL_IN_TRACK": "0"}, []),
]


def pairs(br, defer=0, color=0, layers=0, count=0):
    return "pairs<%d,%d,%d,%d,%d>" % (br, defer, color, layers, count)


# every instantiation kf_integrate_volume can launch in the product build (integrate.hip; not the KF_EXPERIMENTS timing kernels), and every cull
ALL_FUSION = {pairs(1, color=1), pairs(2, color=1), pairs(4, color=1), "bricks<1,1>",
              pairs(1, 1, layers=1), pairs(1, 0, layers=1),
              "pipe<1,1>", "pipe<1,0>", "pipe<0,1>", "pipe<0,0>",
              pairs(1, 1, count=1), pairs(1, 1), pairs(2, 1), pairs(4, 1),
              pairs(1, 0, count=1), pairs(1, 0), pairs(2, 0), pairs(4, 0, count=1), pairs(4, 0),
              "bricks<0,1>", "bricks<0,2>", "bricks<0,4>"}
ALL_CULL = {"tail", "cull<0>", "cull<1>", "cull_sift<0>", "cull_sift<1>"}


def form_name(f):
    if f["kernel"] == K.FUSE_PAIRS:
        return pairs(f["bricks"], f["defer"], f["color"], f["layers"], f["count"])
    if f["kernel"] == K.FUSE_PIPE:
        assert f["bricks"] == 1 and not f["color"] and not f["layers"]
        return "pipe<%d,%d>" % (f["defer"], f["count"])
    if f["kernel"] == K.FUSE_BRICKS:
        assert not f["defer"] and not f["layers"] and not f["count"]
        return "bricks<%d,%d>" % (f["color"], f["bricks"])
    return "none"


def cull_name(f):
    if f["cull"] == K.CULL_TAIL:
        return "tail"
    return {K.CULL_MACRO: "cull<%d>", K.CULL_SIFT: "cull_sift<%d>"}.get(f["cull"], "none%d") % f["cull_defer"]


class Model:
    """kf_integrate_volume's choice (integrate.hip), kf_defer_enabled's and kf_get_volume_stats' bookkeeping of the observed-voxel count (ctx.hip),
    written out again from their documentation: what each frame of a scenario must launch under a switch set"""

    def __init__(self, env, opts):
        g = lambda k, d: int(env[k]) if k in env else d        # noqa: E731  (atoi of the variable, or the default)
        self.br_env = g("KF_INTEGRATE_BR", 0) if g("KF_INTEGRATE_BR", 0) in (1, 2, 4) else 0
        self.cbr = g("KF_INTEGRATE_BR", 2) if g("KF_INTEGRATE_BR", 2) in (1, 2, 4) else 2
        self.pipe = g("KF_INTEGRATE_PIPE", -2)
        self.pairs = g("KF_INTEGRATE_PAIRS", 1)
        self.color_pairs = g("KF_INTEGRATE_COLOR_PAIRS", 1)
        self.sat = g("KF_INTEGRATE_SAT", 1)
        self.sift = g("KF_CULL_SIFT", -1)
        self.count_mode = g("KF_OBSERVED_COUNT", -1)
        self.tail = g("KF_CULL_IN_TRACK", 1)
        grid = g("KF_INTEGRATE_GRID", 1)
        self.grid = grid if 64 <= grid <= 65536 else None
        self.ask_every = "--ask" in opts and opts[opts.index("--ask") + 1] == "every"
        self.set_defer = "--no-set-defer" not in opts

    def frames(self, sc, track_forms):
        """[(fusion form name, cull name, grid or None)] per frame of a scenario"""
        z0, z1 = F.stored_range(sc)
        nb = sc["res"] // 8
        n_bricks = nb * nb * (z1 - z0) // 8
        n_macro = ((nb + 3) // 4) ** 2 * (((z1 // 8 + 3) // 4) - ((z0 // 8) // 4))
        big = n_bricks >= 1 << 20
        override, tracking, valid, asked_before, unasked, hint = -1, False, True, False, 0, False
        out = []
        n = len(sc["frames"])
        for i, fr in enumerate(sc["frames"]):
            if self.set_defer and fr["defer"] is not None:
                override = fr["defer"]
            enabled = bool(self.pairs) and 1.0 <= sc["maxw"] <= 65000.0 and (
                override != 0 if override >= 0 else (self.sat == 2 or (self.sat == 1 and sc["res"] >= 768)))
            defer = enabled and not fr["color"]
            count = tracking and valid
            # the cull: consumed from the tracking launch's tail when the persistent loop ran it for this call's parameters
            tail = sc.get("tracked", False) and hint and self.tail != 0 and not enabled and track_forms[i] == 1
            if tail:
                cull = "tail"
            else:
                sift = self.sift != 0 if self.sift >= 0 else n_macro >= 100000
                cull = ("cull_sift<%d>" if sift else "cull<%d>") % int(defer)
            hint = sc.get("tracked", False)
            counted = False
            if fr["color"]:
                form = pairs(self.cbr, color=1) if self.color_pairs else "bricks<1,1>"
            else:
                br = self.br_env or (4 if big and not defer else 1)
                if self.pairs and fr["layers"]:
                    form = pairs(1, int(defer), layers=1)
                elif self.pairs and br == 1 and (defer if self.pipe < 0 else self.pipe != 0):
                    counted = count
                    form = "pipe<%d,%d>" % (defer, counted)
                elif self.pairs:
                    counted = count and (br == 1 or (br == 4 and not defer))       # (no COUNT instantiation of the others)
                    form = pairs(br, int(defer), count=int(counted))
                else:
                    form = "bricks<0,%d>" % br
            if not counted:
                valid = False
            unasked += 1
            if self.ask_every or i in (0, n - 1):       # kf_get_volume_stats after the frame
                frequent = asked_before and unasked <= 8
                asked_before, unasked = True, 0
                if self.count_mode == 0:
                    tracking = False
                elif self.count_mode == 1 or frequent:
                    tracking = True
                valid = True
            out.append((form, cull, min(n_bricks, self.grid) if self.grid else None))
        return out


@pytest.fixture(scope="module")
def oracle():
    """the oracle's results per scenario (S5's after the first child has reported the poses it tracked)"""
    return {name: F.oracle_run(name, F.SCENARIOS[name]) for name in F.ORDER if not F.SCENARIOS[name].get("tracked")}


_ABORT = []                 # a child that died, hung or failed: no further child is started
_SEEN = {"fusion": set(), "cull": set(), "sets": set(), "started": set()}


def _child_env(env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("KF_") or k in ("KF_STATS_CROSSCHECK", "KF_ORACLE_SO")}
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    return e


@pytest.mark.parametrize("sid,env,opts", SETS, ids=[s[0] for s in SETS])
def test_fusion_form_equals_the_oracle(sid, env, opts, oracle, tmp_path):
    if _ABORT:
        pytest.skip("not started: " + _ABORT[0])
    assert all(k in SWITCHES for k in env), env
    _SEEN["started"].add(sid)
    out = str(tmp_path / "out.npz")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "fusion_forms_child.py"), out] + opts, env=_child_env(env), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _ABORT.append("the child of %s timed out" % sid)
        pytest.fail(_ABORT[0])
    if r.returncode != 0:
        _ABORT.append("the child of %s exited with %d" % (sid, r.returncode))
        pytest.fail(_ABORT[0] + "\n" + r.stderr[-3000:])
    got = np.load(out)
    model = Model(env, opts)
    for name in F.ORDER:
        sc = F.SCENARIOS[name]
        where = (sid, name)
        if sc.get("tracked"):
            poses = got[name + "_pose"]
            if name not in oracle:                      # the oracle fuses with the poses the tracker found (the first switch set's) ...
                oracle[name] = F.oracle_run(name, sc, poses=poses)
                oracle[name]["poses"] = poses
            assert np.array_equal(poses.view(np.uint32), oracle[name]["poses"].view(np.uint32)), where   # ... the same bits under every set
        want = oracle[name]
        assert np.array_equal(got[name + "_upd"], want["upd"]), (where, got[name + "_upd"], want["upd"])
        assert int(want["upd"].sum()) > 10_000, where                 # (there is something to compare)
        asked = got[name + "_gt0"] >= 0
        assert asked.sum() >= 2 and np.array_equal(got[name + "_gt0"][asked], want["gt0"][asked]), (where, got[name + "_gt0"], want["gt0"])
        assert np.array_equal(got[name + "_tsdf"], want["tsdf"].view(np.uint32)), where
        assert np.array_equal(got[name + "_weight"], want["weight"].view(np.uint32)), where
        if want["color"] is not None:
            seen = want["weight"] > 0
            assert np.array_equal(got[name + "_color"][seen], want["color"][seen]), where
            assert int(np.count_nonzero(want["color"][seen])) > 10000, where
        forms = [dict(zip(FORM_FIELDS, (int(x) for x in row))) for row in got[name + "_form"]]
        expect = model.frames(sc, got[name + "_track_form"])
        for i, (f, (fe, ce, ge)) in enumerate(zip(forms, expect)):
            assert (form_name(f), cull_name(f)) == (fe, ce), (where, i, form_name(f), cull_name(f), fe, ce)
            assert f["calls"] == i + 1 and 0 < f["grid"] and (ge is None or f["grid"] == ge), (where, i, f, ge)
            lw = int(got[name + "_layers"][i])
            if sc["frames"][i]["layers"] and f["layers"]:
                assert (lw == want["upd"][i]) if not f["defer"] else (0 < lw <= want["upd"][i]), (where, i, lw, want["upd"][i])
            _SEEN["fusion"].add(form_name(f))
            _SEEN["cull"].add(cull_name(f))
        if sc.get("tracked"):
            consumed = int(got[name + "_tail"][0])
            assert consumed == sum(c == "tail" for _, c, _ in expect), (where, consumed)
    _SEEN["sets"].add(sid)


def test_every_dispatchable_form_ran():
    if _ABORT:
        pytest.skip("not started: " + _ABORT[0])
    if not _SEEN["started"]:
        pytest.skip("no switch set ran in this session (deselected)")
    assert _SEEN["sets"] == {s[0] for s in SETS}, "a switch set failed: " + str(sorted({s[0] for s in SETS} - _SEEN["sets"]))
    assert _SEEN["fusion"] == ALL_FUSION, (sorted(ALL_FUSION - _SEEN["fusion"]), sorted(_SEEN["fusion"] - ALL_FUSION))
    assert _SEEN["cull"] == ALL_CULL, (sorted(ALL_CULL - _SEEN["cull"]), sorted(_SEEN["cull"] - ALL_CULL))
