"""Partial Pose3 factors (Pose3Pose3XYYaw, PriorPose3ZRP; RoME src/factors/PartialPose3.jl) on the host side: the restatement against
the reference's KATs, constructors, packing, the packed-graph tables, the DeviceGraph records, the ABI declarations and the refusals of
the paths that do not serve them.  Runs without a GPU."""
import json
import math
import os
import re
import tempfile

import numpy as np
import pytest

import oracle as ro
import partial3_ref as p3
import rome_jl_amd as R
from rome_jl_amd import serialization
from test_device_graph_plan import GRAPHS, FIXTURE, build, describe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "partialpose3_kats.json")))


# ------------------------------------------------------------------ the restatement reproduces every KAT
def test_kats_mean_measurement():
    m = KATS["mean"]
    assert len(m["cases"]) == 10
    for c in m["cases"]:
        r = p3.residual([m["z"]], [c["p"]], [c["q"]])[0]
        assert np.abs(r - np.array(m["expected"])).max() <= m["atol"] == 1e-12, c["name"]


def test_kats_sign_cases():
    s = KATS["sign"]
    assert len(s["cases"]) == 3
    for c in s["cases"]:
        r = p3.residual([c["z"]], [c.get("p", c.get("p_coords"))], [c.get("q", c.get("q_coords"))])[0]
        assert np.abs(r - np.array(c["expected"])).max() <= s["atol"] == 1e-12, c["name"]


def test_kats_combinations():
    k = KATS["combinations"]
    assert len(k["cases"]) == 14 and k["norm_below"] == 1e-10
    for c in k["cases"]:
        assert np.linalg.norm(p3.residual([c["z"]], [c["p"]], [c["q"]])[0]) < k["norm_below"], c["xyz_rpy"]


def test_yaw_convention():
    assert p3.yaw([0.0, 0.0, 0.7]) == pytest.approx(0.7, abs=1e-16)
    assert p3.yaw_of_point([0, 0, 0, 0.0, 0.0, -1.0, 0, 1, 0, 1, 0, 0]) == 0.0      # the x-axis vertical: atan2(0, 0) = 0
    assert p3.yaw([0.3, 0.0, 0.0]) == 0.0 and abs(p3.yaw([0.0, 0.4, 0.0])) == 0.0     # roll or pitch alone turn no heading


def test_restatement_rows_land_on_roots_and_keep_the_other_coordinates():
    N = 40
    rng = np.random.default_rng(4)
    poses = lambda: np.concatenate([rng.uniform(-40, 40, (3, N)), rng.uniform(-0.35, 0.35, (2, N)), rng.uniform(-math.pi, math.pi, (1, N))])
    oo = ro.make_opts(N=N, solver=1, seed=5)
    fx, tg = poses(), poses()
    cov = np.diag([0.1, 0.1, 0.01]) ** 2
    for d in (0, 1):
        for solver in (p3.NEWTON, p3.GAUSS_NEWTON):
            out, st, z = p3.xyy_row(oo, d, [10.0, 1.0, 0.4], cov, fx, tg, 7, solver)
            r = p3.residual(z, fx.T, out.T) if d == 0 else p3.residual(z, out.T, fx.T)
            assert not st.any() and np.abs(r).max() <= 1e-12 * 50
            assert np.array_equal(out[2:5], tg[2:5])
        out, _, _ = p3.xyy_row(oo, d, [10.0, 1.0, 0.4], cov, fx, tg, 7, p3.NEWTON)
        assert np.abs(out[5]).max() <= math.pi + 0.6     # the principal branch (|w_z| = |psi| up to the tilt's share)
    z = p3.zrp_row(oo, [-10.0, 0.1, -0.2], 0.03, np.diag([0.01, 0.01]) ** 2, tg, 3)
    assert np.array_equal(z[[0, 1, 5]], tg[[0, 1, 5]]) and not np.array_equal(z[2:5], tg[2:5])
    assert abs(z[2].mean() + 10.0) < 0.02 and abs(z[3].mean() - 0.1) < 0.01 and abs(z[4].mean() + 0.2) < 0.01
    # r = p = 0 row: the identity rotation, w = 0
    z0 = p3.zrp_sample([1.0, 0.0, 0.0], 0.0, [1e-3, 0.0, 1e-3], [0.3, 0.0, 0.0])
    assert np.array_equal(z0, [1.0, 0.0, 0.0])


# ------------------------------------------------------------------ factor classes, packing
def test_constructors_and_validation():
    f = R.Pose3Pose3XYYaw(R.MvNormal([20.0, 5.0, math.pi / 2], np.diag([0.01, 0.01, 0.03]) ** 2))
    assert f.partial == (1, 2, 6) and f.variable_types == (R.Pose3, R.Pose3) and not f.is_prior
    g = R.PriorPose3ZRP(R.Normal(-10.0, 0.03), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2))
    assert g.partial == (3, 4, 5) and g.variable_types == (R.Pose3,) and g.is_prior
    with pytest.raises(ValueError):
        R.Pose3Pose3XYYaw(R.MvNormal(np.zeros(6), np.eye(6)))
    with pytest.raises(TypeError):
        R.Pose3Pose3XYYaw(R.Normal(0.0, 1.0))
    with pytest.raises(TypeError):
        R.PriorPose3ZRP(R.MvNormal([0.0], [[1.0]]), R.MvNormal([0.0, 0.0], np.eye(2)))
    with pytest.raises(TypeError):
        R.PriorPose3ZRP(R.Normal(0.0, 1.0), R.Normal(0.0, 1.0))
    with pytest.raises(ValueError):
        R.PriorPose3ZRP(R.Normal(0.0, 1.0), R.MvNormal(np.zeros(3), np.eye(3)))


def test_pack_unpack_roundtrip():
    f = R.Pose3Pose3XYYaw(R.MvNormal([20.0, 5.0, 1.5], np.array([[0.04, 0.01, 0], [0.01, 0.05, 0], [0, 0, 0.001]])))
    d = R.pack_factor(f)
    assert d["fnctype"] == "Pose3Pose3XYYaw" and set(d) == {"fnctype", "Z"}
    f2 = R.unpack_factor(d)
    assert type(f2) is R.Pose3Pose3XYYaw and np.array_equal(f2.Z.mu, f.Z.mu) and np.array_equal(f2.Z.cov, f.Z.cov)
    f3 = serialization.unpackFactor("RoME.PackedPose3Pose3XYYaw", serialization.packFactor(f))
    assert type(f3) is R.Pose3Pose3XYYaw and np.array_equal(f3.Z.cov, f.Z.cov)
    g = R.PriorPose3ZRP(R.Normal(-10.0, 0.03), R.MvNormal([0.1, -0.2], np.array([[0.01, 0.002], [0.002, 0.02]])))
    d = R.pack_factor(g)
    assert d["fnctype"] == "PriorPose3ZRP" and set(d) == {"fnctype", "zdata", "rpdata"}      # the reference's packed field names
    g2 = R.unpack_factor(d)
    assert type(g2) is R.PriorPose3ZRP and (g2.z.mu, g2.z.sigma) == (-10.0, 0.03) and np.array_equal(g2.rp.cov, g.rp.cov)
    pk = serialization.packFactor(g)
    assert set(pk) == {"zdata", "rpdata"}
    g3 = serialization.unpackFactor("RoME.PackedPriorPose3ZRP", pk)
    assert type(g3) is R.PriorPose3ZRP and np.array_equal(g3.rp.mu, g.rp.mu) and np.array_equal(g3.rp.cov, g.rp.cov)


def _graph(N=16, with_partial=True):
    """five poses: a full prior and Pose3Pose3 odometry, plus (with_partial) XYYaw odometry and ZRP priors"""
    fg = R.initfg(N=N)
    for k in range(5):
        fg.addVariable("x%d" % k, R.Pose3)
    fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.diag([0.1] * 3 + [0.01] * 3) ** 2)))
    for k in range(1, 5):
        fg.addFactor(["x%d" % (k - 1), "x%d" % k], R.Pose3Pose3(R.MvNormal([10.0, 0, 0, 0, 0, math.pi / 2], np.diag([0.1] * 3 + [0.01] * 3) ** 2)))
    if with_partial:
        for k in range(1, 5):
            fg.addFactor(["x%d" % k], R.PriorPose3ZRP(R.Normal(float(k), 0.1), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2)),
                         nullhypo=0.25 if k == 3 else None)
        for k in (1, 2, 4):
            fg.addFactor(["x%d" % (k - 1), "x%d" % k], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, math.pi / 2], np.diag([0.1, 0.1, 0.01]) ** 2)),
                         nullhypo=0.5 if k == 2 else None)
    return fg


def _zero_init(fg):
    for l, t in fg.variables.items():
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    return fg


def test_save_load_roundtrip():
    fg = _graph()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "fg.tar.gz")
        R.saveDFG(fg, p)
        fg2 = R.loadDFG(p)
    kx = lambda g: sorted((tuple(l), tuple(f.Z.mu), tuple(f.Z.cov.ravel())) for _, l, f in g.factors if isinstance(f, R.Pose3Pose3XYYaw))
    kz = lambda g: sorted((tuple(l), f.z.mu, f.z.sigma, tuple(f.rp.mu), tuple(f.rp.cov.ravel())) for _, l, f in g.factors if isinstance(f, R.PriorPose3ZRP))
    assert len(kx(fg2)) == 3 and kx(fg2) == kx(fg) and len(kz(fg2)) == 4 and kz(fg2) == kz(fg)


def test_packed_tables():
    fg = _graph()
    pk, pk0 = R.PackedGraph(fg), R.PackedGraph(_graph(with_partial=False))
    ix = pk.index
    xy, zr = pk.p3xyy, pk.zrp3
    assert xy["F"] == 3 and list(xy["var_from"]) == [ix["x0"], ix["x1"], ix["x3"]] and list(xy["var_to"]) == [ix["x1"], ix["x2"], ix["x4"]]
    assert xy["mu"].shape == (3, 3) and xy["cov"].shape == (3, 3, 3) and list(xy["nh"]) == [0.0, 0.5, 0.0]
    assert zr["F"] == 4 and list(zr["var"]) == [ix["x%d" % k] for k in range(1, 5)] and list(zr["nh"]) == [0.0, 0.0, 0.25, 0.0]
    assert zr["mu"].tolist() == [[float(k), 0.0, 0.0] for k in range(1, 5)] and list(zr["sigma_z"]) == [0.1] * 4 and zr["cov_rp"].shape == (4, 2, 2)
    assert pk.has_partial3() and not pk0.has_partial3() and pk0.p3xyy["F"] == 0 and pk0.zrp3["F"] == 0
    for name in ("p3p3", "prior3"):       # the full-factor tables do not see the partial ones
        for k, v in getattr(pk0, name).items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, getattr(pk, name)[k])
    pt = R.PackedGraph.from_pose2_tables(8, 2, np.zeros((1, 3)), np.eye(3)[None], [0], [1])
    assert pt.p3xyy["F"] == 0 and pt.zrp3["F"] == 0 and not pt.has_partial3()


def test_device_graph_records_plan_only():
    """p3xyy then zrp3 as the LAST families, offsets 13 / 14 << 28, their proposal rows behind every other Pose3 row"""
    dg = R.DeviceGraph(_zero_init(_graph()), plan_only=True)
    dg0 = R.DeviceGraph(_zero_init(_graph(with_partial=False)), plan_only=True)
    assert (dg.STREAM_P3XYY, dg.STREAM_ZRP3) == (13 << 28, 14 << 28)
    o = R.make_opts(N=16, solver=1, stream_offset=1000)
    plan, plan0 = dg.conv_plan(o, sweep=3), dg0.conv_plan(o, sweep=3)
    assert plan[:len(plan0)] == plan0                       # nothing about the other launches changes
    tail = plan[len(plan0):]
    assert [p["name"] for p in tail] == ["p3xyy", "zrp3"]
    base = 1000 + (3 << 32)
    assert [p["stream_offset"] for p in tail] == [base + (13 << 28), base + (14 << 28)]
    assert [p["entry"] for p in tail] == ["rome_conv_pose3pose3xyyaw_dev", "rome_conv_priorpose3zrp_dev"]
    assert [p["n_conv"] for p in tail] == [6, 4] and all(p["vt_target"] == "Pose3" and not p["fused"] and p["cols"] == ["nh"] for p in tail)
    n0 = dg0.n_prop[R.Pose3]
    assert [p["prop_lo"] for p in tail] == [n0, n0 + 6] and dg.n_prop[R.Pose3] == n0 + 10
    fams = dg.families(every=True)
    assert fams[-2:] == ["p3xyy", "zrp3"] and fams[:-2] == dg0.families(every=True)
    assert dg.families() == dg0.families() and dg.has_partial3() and not dg0.has_partial3()
    ix = dg.packed.index
    rx, rz = dg.family_table("p3xyy"), dg.family_table("zrp3")
    assert rx["rows4"].tolist() == [[0, 0, ix["x0"], ix["x1"]], [0, 1, ix["x1"], ix["x0"]], [1, 0, ix["x1"], ix["x2"]], [1, 1, ix["x2"], ix["x1"]],
                                    [2, 0, ix["x3"], ix["x4"]], [2, 1, ix["x4"], ix["x3"]]]
    assert rz["rows4"].tolist() == [[k, 0, ix["x%d" % (k + 1)], ix["x%d" % (k + 1)]] for k in range(4)]
    assert rz["vt_fixed"] is R.Pose3 and rz["vt_target"] is R.Pose3 and tuple(rz["L"].shape) == (4, 4) and tuple(rx["L"].shape) == (3, 6)
    assert rx["nh"].tolist() == [0, 0, 0.5, 0.5, 0, 0] and rz["nh"].tolist() == [0, 0, 0.25, 0]
    assert list(dg._prop_targets[R.Pose3][:n0]) == list(dg0._prop_targets[R.Pose3])
    assert list(dg._prop_targets[R.Pose3][n0:]) == [ix[l] for l in ("x1", "x0", "x2", "x1", "x4", "x3", "x1", "x2", "x3", "x4")]


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_recorded_conv_plans_are_unchanged(name):
    want = json.load(open(FIXTURE))[name]
    got = describe(build(name, plan_only=True)[1])
    assert got["plan"] == want["plan"] and got["families"] == want["families"] and got["n_prop"] == want["n_prop"]


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    assert "#define ROME_MI355_VERSION 122" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_residual_pose3pose3xyyaw", "rome_residual_pose3pose3xyyaw_pt", "rome_conv_pose3pose3xyyaw", "rome_conv_priorpose3zrp",
           "rome_conv_pose3pose3xyyaw_dev", "rome_conv_priorpose3zrp_dev"}
    assert new <= declared and new <= set(R._lib.SIGNATURES) and declared == set(R._lib.SIGNATURES)


# ------------------------------------------------------------------ refusals
def _small(factor_kind):
    fg = R.initfg(N=16)
    fg.addVariable("x0", R.Pose3); fg.addVariable("x1", R.Pose3)
    fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.eye(6) * 0.01)))
    fg.addFactor(["x0", "x1"], R.Pose3Pose3(R.MvNormal(np.zeros(6), np.eye(6) * 0.01)))
    if factor_kind == "Pose3Pose3XYYaw":
        fg.addFactor(["x0", "x1"], R.Pose3Pose3XYYaw(R.MvNormal([1.0, 0.0, 0.0], np.eye(3) * 0.01)))
        lbl = [fl for fl, _, f in fg.factors if isinstance(f, R.Pose3Pose3XYYaw)][0]
    else:
        fg.addFactor(["x1"], R.PriorPose3ZRP(R.Normal(0.0, 0.1), R.MvNormal([0.0, 0.0], np.eye(2) * 0.01)))
        lbl = [fl for fl, _, f in fg.factors if isinstance(f, R.PriorPose3ZRP)][0]
    return _zero_init(fg), lbl


@pytest.mark.parametrize("name", ["Pose3Pose3XYYaw", "PriorPose3ZRP"])
def test_refusals_name_the_factor(name):
    fg, lbl = _small(name)
    calls = [
        ("solveTree", lambda: R.solveTree(fg)),
        ("solveTree", lambda: R.solveTree(fg, messages="elimination")),
        ("TreeSolver", lambda: R.TreeSolver(fg)),
        ("DeviceStore", lambda: R.clique.DeviceStore(fg)),
        ("CliqueBatch", lambda: R.CliqueBatch(fg, [(lbl, "x1")])),
        ("initAllOrdered", lambda: R.initAllOrdered(fg)),
        ("initAllOrdered", lambda: R.solveGraph(fg, init="ordered")),
        ("solveGraphParametric", lambda: R.solveGraphParametric(fg)),
    ]
    for where, fn in calls:
        with pytest.raises(TypeError, match=name) as e:
            fn()
        assert where in str(e.value)
    from rome_jl_amd import distributed
    dg = R.DeviceGraph(fg, plan_only=True)
    for cls in (distributed.TargetShardedSweep, distributed.PipelinedSegmentSweep):
        with pytest.raises(TypeError, match=name):
            cls(dg, R._lib.Opts(), None, 1, 0, *([[], None, None] if cls is distributed.PipelinedSegmentSweep else []))
    with pytest.raises((TypeError, ValueError)):      # multihypo over a partial factor
        fg.addFactor(["x0", "x1", "x1"], R.Pose3Pose3XYYaw(R.MvNormal([1.0, 0.0, 0.0], np.eye(3) * 0.01)), multihypo=[1.0, 0.5, 0.5])
    fgr = R.initfg(N=16)      # the range refusals keep their wording beside the new ones
    fgr.addVariable("x0", R.Pose2); fgr.addVariable("l0", R.Point2)
    fgr.addFactor(["x0", "l0"], R.Pose2Point2Range(R.Normal(3.0, 0.1)))
    with pytest.raises(TypeError, match="Pose2Point2Range factors are not supported here"):
        R.TreeSolver(_zero_init(fgr))
