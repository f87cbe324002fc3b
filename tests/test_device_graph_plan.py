"""DeviceGraph's family list without a GPU: the launch list of one conv_step, the proposal-row layout, the CSR and the family
tables of a fixed set of small graphs equal tests/golden/device_graph_plans.json.

The fixture was recorded from the commit BEFORE the family list existed (DeviceGraph with one hand-written sweep method per family):
a recorder outside the repository built the same graphs as `GRAPHS` below on a plan-only DeviceGraph of that commit, replaced its
`_launch` and the library call of `sweep_graph_pose2` by functions that write down their arguments, ran `conv_step(opts, sweep=3)`
and dumped what arrived there next to `n_prop`, `_prop_targets`, `csr` and `family_table()`.  It is NOT produced by the code under
test: launch order, Philox offsets, row layout and the null-ness of the optional columns are what that commit issued."""
import json
import os

import numpy as np
import pytest

import rome_jl_amd as R
from test_range_host import _range_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "device_graph_plans.json")
N = 16
SWEEP, STREAM0 = 3, 1000


def _hexagon():
    return R.dead_reckon_init(R.generateGraph_Hexagonal(N=N), seed=3)


def _beehive_mh():
    """multihypo bearing-range sightings and one multihypo Pose2Pose2 closure (its extra row sits behind the prior rows)"""
    fg = R.synth_beehive_mh(poseCountTarget=14, N=N)
    fg.addFactor(["x13", "x0", "x2"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, np.pi / 3], np.diag([0.01, 0.01, 0.0025]))), multihypo=[1.0, 0.7, 0.3])
    return R.dead_reckon_init(fg, seed=4)


def _manhattan_prefix():
    return R.dead_reckon_init(R.loadG2o(os.path.join(ROOT, "tests", "golden", "manhattan.g2o"), N=N, max_edges=40), seed=1)


def _bearingrange_nullhypo():
    fg = R.initfg(N)
    cov = np.diag([0.1, 0.1, 0.01]) ** 2
    fg.addVariable("x0", R.Pose2); fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([0.0, 0, 0], cov)))
    for k in range(1, 5):
        fg.addVariable("x%d" % k, R.Pose2)
        fg.addFactor(["x%d" % (k - 1), "x%d" % k], R.Pose2Pose2(R.MvNormal([5.0, 0, 0.3], cov)), nullhypo=0.3 if k == 2 else None)
    fg.addVariable("l1", R.Point2)
    fg.addFactor(["x0", "l1"], R.Pose2Point2BearingRange(R.Normal(0, 0.05), R.Normal(10.0, 0.3)))
    fg.addFactor(["x3", "l1"], R.Pose2Point2BearingRange(R.Normal(1.0, 0.05), R.Normal(12.0, 0.3)), nullhypo=0.4)
    return R.dead_reckon_init(fg, seed=3)


def _bearingrange_only():
    """no Pose2Pose2 / PriorPose2 rows at all: the two bearing-range directions are launched on their own"""
    fg = R.initfg(N)
    for l, t in (("x0", R.Pose2), ("x1", R.Pose2), ("l1", R.Point2)):
        fg.addVariable(l, t)
    fg.addFactor(["x0", "l1"], R.Pose2Point2BearingRange(R.Normal(0, 0.05), R.Normal(10.0, 0.3)))
    fg.addFactor(["x1", "l1"], R.Pose2Point2BearingRange(R.Normal(1.0, 0.05), R.Normal(12.0, 0.3)))
    return R.dead_reckon_init(fg, seed=8)


def _landmark_prior():
    """PriorPoint2 rows behind the sightings; x2 and l1 frozen (they keep their proposals' rows out of the CSR)"""
    fg = R.generateGraph_Hexagonal(N=N)
    fg.addFactor(["l1"], R.PriorPoint2(R.MvNormal([20.0, 0.0], np.eye(2))))
    return R.dead_reckon_init(fg, seed=6)


def _helix3d():
    fg = R.synth_helix3d(P=24, N=N)
    R.dead_reckon_init_pose3(fg, seed=2)
    return fg


def _range():
    fg = _range_graph(N)
    R.dead_reckon_init(fg, seed=5)
    rng = np.random.default_rng(9)
    for l, c in (("l0", (0.0, 5.0)), ("l1", (3.0, 5.0)), ("l2", (5.0, 3.0))):
        fg.initVariable(l, np.asarray(c)[:, None] + 0.3 * rng.standard_normal((2, N)))
    return fg


GRAPHS = {"hexagon": (_hexagon, ()), "beehive_mh": (_beehive_mh, ()), "manhattan_prefix": (_manhattan_prefix, ()),
          "bearingrange_nullhypo": (_bearingrange_nullhypo, ()), "bearingrange_only": (_bearingrange_only, ()), "landmark_prior_frozen": (_landmark_prior, ("x2", "l1")),
          "helix3d": (_helix3d, ()), "range": (_range, ())}


def build(name, **kw):
    """-> (fg with beliefs, DeviceGraph) of one fixture graph"""
    make, frozen = GRAPHS[name]
    fg = make()
    dg = R.DeviceGraph(fg, **kw)
    if frozen:
        dg.set_frozen(frozen)
    return fg, dg


def describe(dg):
    ints = lambda a: np.asarray(a).astype(int).tolist()
    vts = (R.Pose2, R.Point2, R.Pose3)
    fams = {}
    for f in dg.families(every=True):
        tb = dg.family_table(f)
        fams[f] = dict(n=tb["n"], dir_all=tb["dir_all"], rows4=None if tb["rows4"] is None else ints(tb["rows4"].numpy()),
                       null=[k for k in ("alt", "w", "nh") if tb[k] is None])
    return dict(plan=dg.conv_plan(R.make_opts(N=N, seed=7, stream_offset=STREAM0), sweep=SWEEP),
                n_prop={vt.name: int(dg.n_prop[vt]) for vt in vts},
                prop_targets={vt.name: ints(dg._prop_targets[vt]) for vt in vts},
                csr={vt.name: dict(ptr=ints(dg.csr[vt]["ptr_h"]), rows=ints(dg.csr[vt]["rows_h"])) for vt in vts},
                families=fams)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_plan_layout_and_tables_equal_the_recorded_ones(name):
    want = json.load(open(FIXTURE))[name]
    got = describe(build(name, plan_only=True)[1])
    for key in ("plan", "n_prop", "prop_targets", "csr", "families"):
        assert got[key] == want[key], key


def test_fixture_takes_every_branch():
    fx = json.load(open(FIXTURE))
    entries = {name: [(p["name"], p["fused"]) for p in g["plan"]] for name, g in fx.items()}
    assert entries["hexagon"] == [("p2p2", True), ("br1", True), ("br0", True)]
    assert entries["bearingrange_only"] == [("br1", False), ("br0", False)]
    assert [n for n, _ in entries["range"]] == ["p2p2", "priorpt2", "p2rng", "pprng1", "pprng0"]
    assert not any(f for _, f in entries["manhattan_prefix"] + entries["helix3d"] + entries["range"])
    cols = {name: {p["name"]: p["cols"] for p in g["plan"]} for name, g in fx.items()}
    assert cols["hexagon"] == {"p2p2": [], "br1": [], "br0": []}   # plain tables: the lean kernels
    assert cols["beehive_mh"] == {"p2p2": ["alt", "w"], "br1": ["alt", "w"], "br0": ["alt", "w"]}
    assert cols["bearingrange_nullhypo"] == {"p2p2": ["nh"], "br1": ["nh"], "br0": ["nh"]}
    assert fx["landmark_prior_frozen"]["families"]["priorpt2"]["rows4"] is None
    assert len(fx["landmark_prior_frozen"]["csr"]["Point2"]["rows"]) == 0   # l1 is frozen
