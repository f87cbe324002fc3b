"""Bearing-only factor (Pose2Point2Bearing; RoME src/factors/Bearing2D.jl) on the host side: constructor, packing, the parametric
measurement, the packed-graph table, the DeviceGraph records, the ABI declarations, the refusals of the paths that do not serve it,
and bearing_ref's own invariants (one-step rules, the reference's residual KATs).  Runs without a GPU."""
import json
import math
import os
import re
import tempfile

import numpy as np
import pytest

import bearing_ref
import oracle as ro
import rome_jl_amd as R
from rome_jl_amd import serialization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "bearing2d_kats.json")))


def test_constructor_defaults_and_types():
    f = R.Pose2Point2Bearing()
    assert isinstance(f.Z, R.Normal) and (f.Z.mu, f.Z.sigma) == (0.0, 1.0)      # Bearing2D.jl:15
    assert f.variable_types == (R.Pose2, R.Point2) and not hasattr(f, "partial")
    g = R.Pose2Point2Bearing(R.Uniform(-1.0, 3.0))
    assert (g.Z.mu, g.Z.sigma) == (1.0, -2.0)
    with pytest.raises(TypeError):
        R.Pose2Point2Bearing(R.MvNormal([1.0], [[1.0]]))
    with pytest.raises(TypeError):
        R.Pose2Point2Bearing(0.3)


def test_pack_unpack_roundtrip():
    for f in (R.Pose2Point2Bearing(R.Normal(0.7, 0.05)), R.Pose2Point2Bearing(R.Uniform(-0.5, 1.5))):
        d = R.pack_factor(f)
        assert d["fnctype"] == "Pose2Point2Bearing" and set(d) == {"fnctype", "Z"}
        g = R.unpack_factor(d)
        assert type(g) is R.Pose2Point2Bearing and (g.Z.mu, g.Z.sigma) == (f.Z.mu, f.Z.sigma)
        h = serialization.unpackFactor("RoME.PackedPose2Point2Bearing", serialization.packFactor(f))
        assert type(h) is R.Pose2Point2Bearing and (h.Z.mu, h.Z.sigma) == (f.Z.mu, f.Z.sigma)


def test_get_measurement_parametric():
    mu, info = R.getMeasurementParametric(R.Pose2Point2Bearing(R.Normal(0.4, 0.05)))
    assert mu.shape == (1,) and info.shape == (1, 1)
    assert mu[0] == 0.4 and info[0, 0] == 1.0 / 0.05 ** 2
    with pytest.raises(TypeError):
        R.getMeasurementParametric(R.Pose2Point2Bearing(R.Uniform(0.0, 1.0)))
    from rome_jl_amd import parametric
    assert parametric._KIND[R.Pose2Point2Bearing] == R._lib.FACTOR_POSE2POINT2BEARING == 6
    assert R.api._LIN_DIMS[6] == (1, 1, 3, 2)


def _bearing_graph(N=20, with_bearing=True):
    """odometry, one bearing-range sighting, a landmark prior, one range factor and (with_bearing) three bearing-only sightings"""
    fg = R.initfg(N=N)
    for l in ("x0", "x1", "x2"):
        fg.addVariable(l, R.Pose2)
    for l in ("l0", "l1"):
        fg.addVariable(l, R.Point2)
    cov = np.diag([0.1, 0.1, 0.01])
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([0.0, 0.0, 0.0], cov)))
    fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, 0.3], cov)))
    fg.addFactor(["x1", "x2"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, 0.3], cov)))
    fg.addFactor(["x0", "l0"], R.Pose2Point2BearingRange(R.Normal(0.5, 0.05), R.Normal(12.0, 0.3)))
    fg.addFactor(["l0"], R.PriorPoint2(R.MvNormal([10.0, 6.0], np.eye(2))))
    fg.addFactor(["x2", "l0"], R.Pose2Point2Range(R.Normal(11.0, 0.3)))
    if with_bearing:
        fg.addFactor(["x0", "l1"], R.Pose2Point2Bearing(R.Normal(0.9, 0.05)))
        fg.addFactor(["x2", "l1"], R.Pose2Point2Bearing(R.Uniform(1.5, 2.5)), nullhypo=0.25)
        fg.addFactor(["x1", "l0"], R.Pose2Point2Bearing(R.Normal(0.2, 0.02)))
    return fg


def _zero_init(fg):
    for l, t in fg.variables.items():
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    return fg


def test_save_load_roundtrip():
    fg = _bearing_graph()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "fg.tar.gz")
        R.saveDFG(fg, p)
        fg2 = R.loadDFG(p)
    key = lambda g: sorted((tuple(l), f.Z.mu, f.Z.sigma) for _, l, f in g.factors if isinstance(f, R.Pose2Point2Bearing))
    assert len(key(fg2)) == 3 and key(fg2) == key(fg)


def test_packed_graph_table():
    fg = _bearing_graph()
    pk = R.PackedGraph(fg)
    ix, pb = pk.index, pk.pbear
    assert set(pb) == {"F", "mu", "sigma", "pose", "point", "nh", "labels"} and pb["F"] == 3
    assert list(pb["pose"]) == [ix["x0"], ix["x2"], ix["x1"]] and list(pb["point"]) == [ix["l1"], ix["l1"], ix["l0"]]
    assert list(pb["mu"]) == [0.9, 2.0, 0.2] and list(pb["sigma"]) == [0.05, -0.5, 0.02] and list(pb["nh"]) == [0.0, 0.25, 0.0]
    assert pk.has_bearing() and pk.has_range()
    pk0 = R.PackedGraph(_bearing_graph(with_bearing=False))
    assert pk0.pbear["F"] == 0 and not pk0.has_bearing()
    for name in ("p2p2", "prior2", "priorpt2", "pprng"):      # the other tables do not see the bearing-only factors
        for k, v in getattr(pk0, name).items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, getattr(pk, name)[k])


def test_device_graph_records_plan_only():
    """pb1 then pb0 as the LAST launches, offsets 11 / 12 << 28, their proposal rows behind every earlier family's"""
    dg = R.DeviceGraph(_zero_init(_bearing_graph()), plan_only=True)
    dg0 = R.DeviceGraph(_zero_init(_bearing_graph(with_bearing=False)), plan_only=True)
    assert (dg.STREAM_PB1, dg.STREAM_PB0) == (11 << 28, 12 << 28)
    o = R.make_opts(N=20, solver=1, stream_offset=1000)
    plan, plan0 = dg.conv_plan(o, sweep=3), dg0.conv_plan(o, sweep=3)
    assert plan[:len(plan0)] == plan0                       # nothing about the other launches changes
    tail = plan[len(plan0):]
    assert [p["name"] for p in tail] == ["pb1", "pb0"]
    base = 1000 + (3 << 32)
    assert [p["stream_offset"] for p in tail] == [base + (11 << 28), base + (12 << 28)]
    assert all(p["entry"] == "rome_conv_pose2point2bearing_dev" and p["n_conv"] == 3 and not p["fused"] and p["cols"] == ["nh"] for p in tail)
    assert [p["dir_all"] for p in tail] == [1, 0] and [p["vt_target"] for p in tail] == ["Pose2", "Point2"]
    assert tail[0]["prop_lo"] == dg0.n_prop[R.Pose2] and tail[1]["prop_lo"] == dg0.n_prop[R.Point2]
    assert dg.n_prop[R.Pose2] == dg0.n_prop[R.Pose2] + 3 and dg.n_prop[R.Point2] == dg0.n_prop[R.Point2] + 3
    ix = dg.packed.index
    assert list(dg._prop_targets[R.Pose2][-3:]) == [ix["x0"], ix["x2"], ix["x1"]]
    assert list(dg._prop_targets[R.Point2][-3:]) == [ix["l1"], ix["l1"], ix["l0"]]
    assert list(dg._prop_targets[R.Pose2][:-3]) == list(dg0._prop_targets[R.Pose2])
    fams = dg.families(every=True)          # appended right after pprng0 (the prior samplers behind own no proposal rows)
    assert fams[fams.index("pprng0") + 1:fams.index("pprng0") + 3] == ["pb1", "pb0"]
    assert [f for f in fams if f not in ("pb1", "pb0")] == dg0.families(every=True)
    assert dg.has_bearing() and dg.has_range() and not dg0.has_bearing()
    assert dg.families() == dg0.families()
    r1, r0 = dg.family_table("pb1"), dg.family_table("pb0")
    assert r1["rows4"].tolist() == [[0, 1, ix["l1"], ix["x0"]], [1, 1, ix["l1"], ix["x2"]], [2, 1, ix["l0"], ix["x1"]]]
    assert r0["rows4"].tolist() == [[0, 0, ix["x0"], ix["l1"]], [1, 0, ix["x2"], ix["l1"]], [2, 0, ix["x1"], ix["l0"]]]


def test_header_declares_the_bearing_entries():
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    assert "ROME_FACTOR_POSE2POINT2BEARING = 6" in hdr and "#define ROME_MI355_VERSION 122" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_residual_pose2point2bearing", "rome_residual_pose2point2bearing_pt", "rome_conv_pose2point2bearing",
           "rome_conv_pose2point2bearing_dev"}
    assert new <= declared and new <= set(R._lib.SIGNATURES)
    assert declared == set(R._lib.SIGNATURES)


def test_refusals_without_a_device():
    fg = R.initfg(N=20)
    fg.addVariable("x0", R.Pose2); fg.addVariable("l0", R.Point2); fg.addVariable("l1", R.Point2)
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([0.0, 0.0, 0.0], np.diag([0.1, 0.1, 0.01]))))
    fg.addFactor(["x0", "l0"], R.Pose2Point2Bearing(R.Normal(0.3, 0.05)))
    _zero_init(fg)
    calls = [
        ("solveTree", lambda: R.solveTree(fg)),
        ("solveTree", lambda: R.solveTree(fg, messages="elimination")),
        ("TreeSolver", lambda: R.TreeSolver(fg)),
        ("DeviceStore", lambda: R.clique.DeviceStore(fg)),
        ("CliqueBatch", lambda: R.CliqueBatch(fg, [("x0l0f1", "l0")])),
        ("initAllOrdered", lambda: R.initAllOrdered(fg)),
        ("initAllOrdered", lambda: R.solveGraph(fg, init="ordered")),
    ]
    for where, fn in calls:
        with pytest.raises(TypeError, match="Pose2Point2Bearing") as e:
            fn()
        assert where in str(e.value)
    from rome_jl_amd import distributed
    dg = R.DeviceGraph(fg, plan_only=True)
    for cls in (distributed.TargetShardedSweep, distributed.PipelinedSegmentSweep):
        with pytest.raises(TypeError, match="Pose2Point2Bearing"):
            cls(dg, R._lib.Opts(), None, 1, 0, *([[], None, None] if cls is distributed.PipelinedSegmentSweep else []))
    # multihypo over a bearing-only sighting
    with pytest.raises((TypeError, ValueError)):
        fg.addFactor(["x0", "l0", "l1"], R.Pose2Point2Bearing(R.Normal(0.3, 0.05)), multihypo=[1.0, 0.5, 0.5])
    # the range refusals keep their wording beside the new ones
    fgr = R.initfg(N=20)
    fgr.addVariable("x0", R.Pose2); fgr.addVariable("l0", R.Point2)
    fgr.addFactor(["x0", "l0"], R.Pose2Point2Range(R.Normal(3.0, 0.1)))
    with pytest.raises(TypeError, match="Pose2Point2Range factors are not supported here"):
        R.TreeSolver(_zero_init(fgr))


def test_bearing_ref_one_step_rules_land_on_a_root():
    rng = np.random.default_rng(3)
    n = 2000
    b = rng.uniform(-4, 4, n)
    pose = np.column_stack([rng.uniform(-40, 40, (n, 2)), rng.uniform(-3.2, 3.2, n)])
    lm = rng.uniform(-40, 40, (n, 2))
    t0 = np.array([bearing_ref.step(b[i], pose[i], lm[i]) for i in range(n)])            # landmark from the fixed pose
    assert np.abs(bearing_ref.residual(b, pose, t0)).max() <= 1e-12
    assert np.allclose(np.hypot(*(t0 - pose[:, :2]).T), np.hypot(*(lm - pose[:, :2]).T), rtol=1e-14, atol=0)   # the distance is kept
    t1 = np.array([bearing_ref.step(b[i], lm[i], pose[i]) for i in range(n)])            # pose from the fixed landmark
    assert np.abs(bearing_ref.residual(b, t1, lm)).max() <= 1e-12
    assert np.array_equal(t1[:, :2], pose[:, :2]) and np.abs(t1[:, 2]).max() <= math.pi   # the translation is kept bit for bit
    # degenerate rows: the start on the anchor
    assert np.array_equal(bearing_ref.step(0.7, [1.0, 2.0, 0.4], [1.0, 2.0]), [1.0, 2.0])
    assert np.array_equal(bearing_ref.step(4.0, [1.0, 2.0], [1.0, 2.0, 0.4]), [1.0, 2.0, bearing_ref.wrap(-4.0)])


def test_bearing_ref_convolution_invariants():
    N = 40
    rng = np.random.default_rng(8)
    oo = ro.make_opts(N=N, solver=0, seed=11, inflate_cycles=3, inflation=5.0)
    pts = rng.uniform(-10, 10, (2, 2, N))
    poses = np.concatenate([rng.uniform(10, 30, (2, 2, N)), rng.uniform(-3, 3, (2, 1, N))], axis=1)
    mu, sigma = np.array([0.5, -2.0]), np.array([0.05, -0.4])
    for fixed, target in ((poses, pts), (pts, poses)):
        for solver in (bearing_ref.CLOSED_FORM, bearing_ref.NEWTON, bearing_ref.GAUSS_NEWTON):
            out, st = bearing_ref.conv(oo, mu, sigma, fixed, target, solver)
            assert not st.any()
            for c in range(2):
                b = np.array([bearing_ref.measurement(mu[c], sigma[c], ro.rng_normals(11, c, i, 1)[0]) for i in range(N)])
                pose, lm = (fixed[c].T, out[c].T) if target.shape[1] == 2 else (out[c].T, fixed[c].T)
                assert np.abs(bearing_ref.residual(b, pose, lm)).max() <= 1e-12
        # a pose target keeps its (jittered) translation: two rows that differ only in mu return the same (x, y) after ONE cycle (from
        # the second cycle on the compose-form jitter is rotated by the heading the first solve set, which depends on mu), and
        # without inflation the start translations come back bit for bit after any number of cycles
        if target.shape[1] == 3:
            o1 = ro.make_opts(N=N, solver=0, seed=11, inflate_cycles=1, inflation=5.0)
            a, _ = bearing_ref.conv_row(o1, 0.5, 0.05, fixed[0], target[0], 5, bearing_ref.NEWTON)
            b_, _ = bearing_ref.conv_row(o1, -1.5, 0.05, fixed[0], target[0], 5, bearing_ref.NEWTON)
            assert np.array_equal(a[:2], b_[:2]) and not np.array_equal(a[2], b_[2]) and not np.array_equal(a[:2], target[0, :2])
            o0 = ro.make_opts(N=N, solver=0, seed=11, inflate_cycles=3, inflation=0.0)
            a, _ = bearing_ref.conv_row(o0, 0.5, 0.05, fixed[0], target[0], 5, bearing_ref.NEWTON)
            assert np.array_equal(a[:2], target[0, :2])


def test_reference_kats_against_bearing_ref():
    g = KATS["grid"]
    poses = np.array(g["poses"])
    r = bearing_ref.residual(np.full(len(poses), g["b"]), poses, np.tile(g["q"], (len(poses), 1)))
    d = np.array([ro.sym_rem(x) for x in r - np.array(g["expected"])])
    assert len(poses) == 11 and np.abs(d).max() <= g["atol"]
    for k in ("sign", "pm_pi"):
        c = KATS[k]
        r = bearing_ref.residual([c["b"]], [c["pose"]], [c["l"]])[0]
        assert abs(r - c["expected"]) <= c["atol"], (k, r)


def test_sharded_parametric_solve_refuses_by_name():
    fg = R.initfg(N=20)
    fg.addVariable("x0", R.Pose2); fg.addVariable("l0", R.Point2)
    fg.addFactor(["x0", "l0"], R.Pose2Point2Bearing(R.Normal(0.3, 0.05)))
    with pytest.raises(TypeError, match="Pose2Point2Bearing"):
        R.solveGraphParametric(fg, shard=object())
