"""Range-only factors (Point2Point2Range, Pose2Point2Range; RoME src/factors/Range2D.jl) on the host side: constructors, packing,
the packed-graph tables, the ABI declarations, the refusals of the paths that do not serve them, and range_ref's own invariants.
Runs without a GPU."""
import json
import os
import re
import tempfile

import numpy as np
import pytest

import oracle as ro
import range_ref
import rome_jl_amd as R
from rome_jl_amd import serialization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructors_and_types():
    f = R.Point2Point2Range(R.Normal(100.0, 1.0))
    assert f.variable_types == (R.Point2, R.Point2) and f.Z.mu == 100.0
    g = R.Pose2Point2Range(R.Uniform(4.0, 6.0))
    assert g.variable_types == (R.Pose2, R.Point2) and g.partial == (1, 2) and g.Z.sigma == -1.0
    for cls in (R.Point2Point2Range, R.Pose2Point2Range):
        with pytest.raises(TypeError):
            cls(R.MvNormal([1.0], [[1.0]]))
        with pytest.raises(TypeError):
            cls(3.0)


def test_pack_unpack_roundtrip():
    for f in (R.Point2Point2Range(R.Normal(12.5, 0.25)), R.Pose2Point2Range(R.Uniform(1.0, 3.0))):
        g = R.unpack_factor(R.pack_factor(f))
        assert type(g) is type(f) and (g.Z.mu, g.Z.sigma) == (f.Z.mu, f.Z.sigma)
        h = serialization.unpackFactor("RoME.Packed" + type(f).__name__, serialization.packFactor(f))
        assert type(h) is type(f) and (h.Z.mu, h.Z.sigma) == (f.Z.mu, f.Z.sigma)


def test_unpack_reference_packed_record():
    """test/testPoint2Point2.jl:103-140 (RoME issue #563): the reference's packed Point2Point2Range factor record"""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "point2point2range_packed.json")))
    data = json.loads(rec["data"])
    f = serialization.unpackFactor(rec["fnctype"], data["fnc"])
    assert isinstance(f, R.Point2Point2Range)
    assert isinstance(f.Z, R.Normal) and f.Z.mu == 89.44271909999159 and f.Z.sigma == 3.0
    fg = R.initfg(N=10)
    fg.addVariable("x0", R.Point2); fg.addVariable("l3", R.Point2)
    fg.addFactor(rec["_variableOrderSymbols"], f)


def _range_graph(N=20):
    fg = R.initfg(N=N)
    for l in ("x0", "x1"):
        fg.addVariable(l, R.Pose2)
    for l in ("l0", "l1", "l2"):
        fg.addVariable(l, R.Point2)
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([0.0, 0.0, 0.0], np.diag([0.1, 0.1, 0.01]))))
    fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([1.0, 0.0, 0.0], np.diag([0.1, 0.1, 0.01]))))
    fg.addFactor(["l0"], R.PriorPoint2(R.MvNormal([0.0, 5.0], np.eye(2))))
    fg.addFactor(["l0", "l1"], R.Point2Point2Range(R.Normal(3.0, 0.1)))
    fg.addFactor(["l2", "l1"], R.Point2Point2Range(R.Uniform(2.0, 4.0)), nullhypo=0.25)
    fg.addFactor(["x1", "l2"], R.Pose2Point2Range(R.Normal(5.0, 0.2)))
    return fg


def test_save_load_roundtrip():
    fg = _range_graph()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "fg.tar.gz")
        R.saveDFG(fg, p)
        fg2 = R.loadDFG(p)
    got = {type(f).__name__: f for _, _, f in fg2.factors}
    assert isinstance(got["Point2Point2Range"], R.Point2Point2Range) and isinstance(got["Pose2Point2Range"], R.Pose2Point2Range)
    ranges = sorted((l, f.Z.mu, f.Z.sigma) for _, l, f in fg2.factors if isinstance(f, (R.Point2Point2Range, R.Pose2Point2Range)))
    assert ranges == sorted((l, f.Z.mu, f.Z.sigma) for _, l, f in fg.factors if isinstance(f, (R.Point2Point2Range, R.Pose2Point2Range)))


def test_packed_graph_tables_and_rows():
    fg = _range_graph()
    pk = R.PackedGraph(fg)
    ix = pk.index
    r2, rp = pk.p2rng, pk.pprng
    assert r2["F"] == 2 and rp["F"] == 1
    assert list(r2["from"]) == [ix["l0"], ix["l2"]] and list(r2["to"]) == [ix["l1"], ix["l1"]]
    assert list(r2["mu"]) == [3.0, 3.0] and list(r2["sigma"]) == [0.1, -1.0] and list(r2["nh"]) == [0.0, 0.25]
    assert list(rp["pose"]) == [ix["x1"]] and list(rp["point"]) == [ix["l2"]] and list(rp["mu"]) == [5.0]
    factor, dr, fixed, target = R.PackedGraph.range_conv_table(r2)
    assert list(factor) == [0, 0, 1, 1] and list(dr) == [0, 1, 0, 1]
    assert list(fixed) == [ix["l0"], ix["l1"], ix["l2"], ix["l1"]] and list(target) == [ix["l1"], ix["l0"], ix["l1"], ix["l2"]]
    assert pk.has_range()
    # the existing tables are unchanged by the range factors
    fg0 = R.initfg(N=20)
    for l, t in fg.variables.items():
        fg0.addVariable(l, t)
    for _, labels, f in fg.factors:
        if not isinstance(f, (R.Point2Point2Range, R.Pose2Point2Range)):
            fg0.addFactor(labels, f)
    pk0 = R.PackedGraph(fg0)
    assert not pk0.has_range()
    for name in ("p2p2", "prior2", "priorpt2"):
        for k, v in getattr(pk0, name).items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, getattr(pk, name)[k])


def test_device_graph_rows_and_streams_plan_only():
    """proposal rows behind the existing ones and the new Philox family offsets (a plan-only DeviceGraph: no device needed)"""
    fg = _range_graph()
    for l, t in fg.variables.items():
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    dg = R.DeviceGraph(fg, plan_only=True)
    ix = dg.packed.index
    assert (dg.STREAM_P2RNG, dg.STREAM_PPRNG1, dg.STREAM_PPRNG0) == (8 << 28, 9 << 28, 10 << 28)
    assert (dg.STREAM_P2P2, dg.STREAM_BR1, dg.STREAM_BR0, dg.STREAM_PRIORPT2) == (0, 1 << 28, 2 << 28, 7 << 28)
    # Point2: [br0 (none) | priorpt2 (l0) | p2rng rows 2f+dir | pprng dir 0];  Pose2: [p2p2 + prior rows | br1 (none) | pprng dir 1]
    assert list(dg._prop_targets[R.Point2]) == [ix["l0"], ix["l1"], ix["l0"], ix["l1"], ix["l2"], ix["l2"]]
    assert list(dg._prop_targets[R.Pose2]) == [ix["x1"], ix["x0"], ix["x0"], ix["x1"]]
    assert dg.n_prop[R.Point2] == 6 and dg.n_prop[R.Pose2] == 4
    csr = dg.csr[R.Point2]
    assert list(csr["ptr_h"]) == [0, 2, 4, 6]
    assert dg.has_range() and dg.families() == ["p2p2"]


def test_header_declares_the_range_entries():
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_residual_point2point2range", "rome_residual_pose2point2range", "rome_conv_point2point2range",
           "rome_conv_pose2point2range", "rome_conv_point2point2range_dev", "rome_conv_pose2point2range_dev"}
    assert new <= declared and new <= set(R._lib.SIGNATURES)
    assert declared == set(R._lib.SIGNATURES)


def test_refusals_without_a_device():
    fg = _range_graph()
    for l, t in fg.variables.items():
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    calls = [
        ("solveTree", lambda: R.solveTree(fg)),
        ("solveTree", lambda: R.solveTree(fg, messages="elimination")),
        ("solveTree", lambda: R.solveTree(fg, messages="relative")),
        ("TreeSolver", lambda: R.TreeSolver(fg)),
        ("DeviceStore", lambda: R.clique.DeviceStore(fg)),
        ("CliqueBatch", lambda: R.CliqueBatch(fg, [("l0l1f1", "l1")])),
        ("initAllOrdered", lambda: R.initAllOrdered(fg)),
        ("initAllOrdered", lambda: R.solveGraph(fg, init="ordered")),
        ("solveGraphParametric", lambda: R.solveGraphParametric(fg)),
    ]
    for where, fn in calls:
        with pytest.raises(TypeError, match="Range") as e:
            fn()
        assert where in str(e.value)
    from rome_jl_amd import distributed
    dg = R.DeviceGraph(fg, plan_only=True)
    for cls in (distributed.TargetShardedSweep, distributed.PipelinedSegmentSweep):
        with pytest.raises(TypeError, match="Point2Point2Range"):
            cls(dg, R._lib.Opts(), None, 1, 0, *([[], None, None] if cls is distributed.PipelinedSegmentSweep else []))


def test_range_ref_closed_form_on_ring_and_heading_kept():
    N = 40
    rng = np.random.default_rng(8)
    oo = ro.make_opts(N=N, solver=0, seed=11, inflate_cycles=3, inflation=5.0)
    fixed_pt = rng.uniform(-10, 10, (2, 2, N))
    fixed_pose = np.concatenate([fixed_pt, rng.uniform(-3, 3, (2, 1, N))], axis=1)
    target_pose = np.concatenate([rng.uniform(-10, 10, (2, 2, N)), rng.uniform(-9, 9, (2, 1, N))], axis=1)
    mu, sigma = np.array([5.0, 8.0]), np.array([0.5, -1.0])
    for fixed, target in ((fixed_pt, fixed_pt[::-1].copy()), (fixed_pose, fixed_pt[::-1].copy()), (fixed_pt, target_pose)):
        for solver in (range_ref.CLOSED_FORM, range_ref.NEWTON, range_ref.GAUSS_NEWTON):
            out, st = range_ref.conv(oo, mu, sigma, fixed, target, solver)
            for c in range(2):
                rho = [range_ref.measurement(mu[c], sigma[c], ro.rng_normals(11, c, i, 1)[0]) for i in range(N)]
                r = np.array([range_ref.residual(rho[i], fixed[c, :2, i], out[c, :, i]) for i in range(N)])
                assert np.abs(r).max() < 1e-9
            if target.shape[1] == 3:
                assert np.array_equal(out[:, 2], target[:, 2])
            if solver != range_ref.CLOSED_FORM:
                assert not st.any()


def test_range_ref_degenerate_rows():
    a = np.array([1.0, 2.0])
    assert np.array_equal(range_ref.project(-1.0, a, a + 3), a)
    assert np.array_equal(range_ref.project(0.0, a, a + 3), a)
    assert np.array_equal(range_ref.project(2.0, a, a.copy()), a + [2.0, 0.0])
    assert np.allclose(range_ref.project(5.0, a, a + [3.0, 4.0]), a + [3.0, 4.0])
