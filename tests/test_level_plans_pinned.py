"""The host layer of `solveTree` (levels.py, tree.TreeSolver, elimination.RelativeEliminationSolver, clique.UpsolvePlan), pinned without
a GPU.

1. Plan identity: tests/golden/level_plans.json holds, per case of scripts/level_plan_fingerprint.py (Manhattan-3500, the hexagon, a
   bearing-range graph, a multihypo beehive, a Pose3 helix; both TreeSolver forms, the message tree with sweeps and staged products, the
   elimination with two structures and with the star-mesh transform), one digest per step that the solver hands its backend -- the level
   graph in insertion order, every lifted factor and hypothesis, the whole LevelSpec, every block operation -- and one of the lifted
   universe, recorded at the commit before levels.py existed.  Lifted labels, row order (the Philox stream ids) and universe order (the
   block indices) all enter the digests: the solvers must keep handing over exactly that.
2. The two construction paths of UpsolvePlan (frontal lists; a LevelSpec through tree.TreeLevelPlan) fill the same
   rome_clique_upsolve_host for the same frontier, whole and as the shares of a two-clique frontier.  The `<family>_stream` columns are
   compared by what they mean (no column = every row draws its own index), and their FORM is pinned too: a frontier plan passes the
   column even when whole, a whole level passes none -- what each path has always handed the library, and what decides which
   convolution kernel serves the table (csrc/rome_kernels.h, ConvArgs.row_stream)."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rome_jl_amd as R   # noqa: E402
from rome_jl_amd.clique import CliqueUpsolveHost, fill_upsolve_plan, frontier_order, frontier_pairs, plan_frontier, plan_level   # noqa: E402
from rome_jl_amd.levels import LevelSpec   # noqa: E402

_spec = importlib.util.spec_from_file_location("level_plan_fingerprint", os.path.join(ROOT, "scripts", "level_plan_fingerprint.py"))
FP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FP)

with open(os.path.join(ROOT, "tests", "golden", "level_plans.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_pinned_cases_are_the_scripts_cases():
    assert sorted(GOLDEN) == sorted(FP.CASES)


@pytest.mark.parametrize("case", sorted(FP.CASES))
def test_level_plans_are_what_they_were(case):
    got, want = FP.fingerprint(case), GOLDEN[case]
    first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), None)
    assert first is None, "%s: step %d of %d differs (the last entry is the universe)" % (case, first, len(want) - 1)
    assert len(got) == len(want)


# ------------------------------------------------------------------------------------------------ UpsolvePlan: one fill, two paths
def _chain():
    """6 poses, odometry, a prior on x0, the loop closure x5 -> x1; every variable initialised"""
    N = 32
    fg = R.initfg(N)
    rng = np.random.default_rng(3)
    for k in range(6):
        fg.addVariable("x%d" % k, R.Pose2)
        fg.initVariable("x%d" % k, np.array([[k], [0.0], [0.0]]) + 0.1 * rng.standard_normal((3, N)))
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal(np.zeros(3), np.diag([0.01, 0.01, 0.001]))))
    for k in range(5):
        fg.addFactor(["x%d" % k, "x%d" % (k + 1)], R.Pose2Pose2(R.MvNormal([1.0, 0.0, 0.0], np.diag([0.01, 0.01, 0.001]))))
    fg.addFactor(["x5", "x1"], R.Pose2Pose2(R.MvNormal([-4.0, 0.0, 0.0], np.diag([0.02, 0.02, 0.002]))))
    return fg


def _tables(fg, d, mirror=None):
    """every array that `fill_upsolve_plan` hands the library for the description d, by field name"""
    index = {l: k for k, l in enumerate(fg.variables)}          # (one variable type: DeviceStore.index)
    u, keep = CliqueUpsolveHost(), []
    fill_upsolve_plan(u, keep, fg, index, d, mirror)
    q = u.clique

    def arr(ptr, n, ct=C.c_int32):
        return None if not ptr else np.array((ct * n).from_address(ptr))
    out = dict(n_up=u.n_up, gibbs_iters=u.gibbs_iters, product_iters=u.product_iters, schedule=u.schedule,
               n_smsg=(u.n_smsg_pose2, u.n_smsg_point2, u.n_smsg_pose3))
    for name in ("up_type", "up_var", "up_group", "up_stream", "up_mirror"):
        out[name] = arr(getattr(u, name), u.n_up)
    for fam, n, f, dm, dc in (("p2p2", q.n_p2p2, q.f_p2p2, 3, 9), ("br1", q.n_br1, q.f_br, 0, 0), ("br0", q.n_br0, q.f_br, 0, 0),
                              ("p3p3", q.n_p3p3, q.f_p3p3, 6, 36), ("prpt2", q.n_prpt2, q.f_prpt2, 2, 4)):
        out["n_" + fam] = (n, f)
        out[fam + "_rows4"] = arr(getattr(q, fam + "_rows4"), 4 * n)
        sid = arr(getattr(q, fam + "_stream"), n)
        out[fam + "_has_stream_column"] = sid is not None
        out[fam + "_stream"] = np.arange(n, dtype=np.int32) if sid is None else sid      # (NULL: row r draws stream r)
        if dm:
            out[fam + "_mu"] = arr(getattr(q, fam + "_mu"), dm * f, C.c_double)
            out[fam + "_cov"] = arr(getattr(q, fam + "_cov"), dc * f, C.c_double)
    out["br_mu"], out["br_sigma"] = arr(q.br_mu, 2 * q.f_br, C.c_double), arr(q.br_sigma, 2 * q.f_br, C.c_double)
    return out


@pytest.mark.parametrize("cliques,share", [([["x0", "x1", "x2", "x3", "x4", "x5"]], None),      # one clique: six update groups
                                           ([["x1", "x2"], ["x4"]], None), ([["x1", "x2"], ["x4"]], [0]), ([["x1", "x2"], ["x4"]], [1])])
def test_frontal_lists_and_the_equivalent_level_spec_fill_the_same_tables(cliques, share):
    fg = _chain()
    order, _ = frontier_order(cliques)
    pairs = frontier_pairs(fg, cliques, order)
    spec = LevelSpec(fg, [(c, list(range(len(c)))) for c in cliques], {l: [fl for fl, dst in pairs if dst == l] for l in order}, [], 2)
    index = {l: k for k, l in enumerate(fg.variables)}
    mirror = {l: k for k, l in enumerate(order)}
    a = _tables(fg, plan_frontier(fg, cliques, share, var_index=index, gibbs_iters=2), mirror)
    b = _tables(fg, plan_level(spec, share, index), mirror)
    assert a.keys() == b.keys()
    for k in a:
        if not k.endswith("_has_stream_column"):
            assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert a["p2p2_has_stream_column"] and b["p2p2_has_stream_column"] == (share is not None)
    n_up = sum(len(c) for k, c in enumerate(cliques) if share is None or k in share)
    assert a["n_up"] == n_up and a["n_p2p2"][0] > 0 and a["up_stream"] is not None
    if share == [1]:    # x4 is entry 1 of [x1, x4, x2]; its two rows follow the three of x1 in the whole p2p2 table
        assert a["up_stream"].tolist() == [1] and a["p2p2_stream"].tolist() == [3, 4]
