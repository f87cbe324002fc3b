"""Pose3Pose3Rotation (RoME src/factors/PartialPose3.jl:204-227) on the host side: the references of tests/rotation3_ref.py against each
other and against the reference's KATs, the factor class, packing, the DeviceGraph records, the partial-aware product's tasks, the ABI
declarations and the refusals of the paths that do not serve partial Pose3 factors.  Runs without a GPU."""
import json
import math
import os
import re
import tempfile

import numpy as np
import pytest

import lin_ref
import rotation3_ref as r3
import rome_jl_amd as R
from rome_jl_amd import serialization
from rome_jl_amd.factors import partial_coverage, PARTIAL3_FACTORS
from test_device_graph_plan import GRAPHS, FIXTURE, build, describe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "rotation3_kats.json")))
COV = np.diag([0.02, 0.02, 0.02]) ** 2


# ------------------------------------------------------------------ the references
def test_mp_is_finite_on_every_table_row():
    refs = r3.residual_references()
    assert set(refs) == {"phi_tiny", "phi_mid", "near_pi_1e-3", "pose_coords", "generic"}
    for name, (t, co, pt) in refs.items():
        assert np.isfinite(co.ref).all() and np.isfinite(pt.ref).all() and co.ref.shape == t["z"].shape, name
    rt, rr = r3.root_reference()
    assert np.isfinite(rr.ref).all() and len(rr.ref) == 48 and np.abs(rt["z"]).max() <= 3.0
    assert (np.linalg.norm(rr.ref, axis=1) <= math.pi).all()                     # principal rotation vectors


def test_tables_hold_the_angles_they_name():
    for name, (t, co, _) in r3.residual_references().items():
        if name in r3.RESIDUAL_ANGLES:
            ang = np.linalg.norm(t["z"] - co.ref, axis=1)                        # |Log(R_p^T R_q)|
            want = np.tile(r3.RESIDUAL_ANGLES[name], len(lin_ref.AXES))
            assert np.abs(ang - want).max() <= 1e-12, name
    t = r3.residual_references()["pose_coords"][0]
    norms = sorted(set(np.round(np.linalg.norm(np.concatenate([t["p"][0::2, 3:], t["q"][1::2, 3:]]), axis=1), 9)))
    assert np.allclose(norms, sorted(lin_ref.POSE_NORMS), atol=1e-8)


def test_restatement_against_mp():
    """the float64 restatement's deviation from mp: rounding level everywhere but where the shared log formula sqrt(1 - c^2)/acos(c) loses
    digits, and there under its worst case (lin_ref.log_formula_error)"""
    for name, (t, co, pt) in r3.residual_references().items():
        for side in (co, pt):
            cap = 64 * lin_ref.EPS
            if name == "phi_mid":
                cap = lin_ref.log_formula_error(3.0)
            if name == "near_pi_1e-3":
                cap = lin_ref.log_formula_error(math.pi - 1e-3)
            print("%s: figure %.3e (cap %.3e), kernel bound %.3e" % (name, side.figure, cap, side.rel_bound))
            assert side.figure <= cap, name
            assert side.rel_bound == max(8 * side.figure, 64 * lin_ref.EPS)
    rt, rr = r3.root_reference()
    print("roots: figure %.3e, kernel bound %.3e" % (rr.figure, rr.rel_bound))
    assert rr.figure <= 64 * lin_ref.EPS
    # the root is the zero of the functor (|z| <= 3 < pi), in mp on both sides
    tg = np.concatenate([np.zeros((48, 3)), rr.ref], axis=1)
    p = np.where(rt["dirs"][:, None] == 0, rt["fixed"], tg)
    q = np.where(rt["dirs"][:, None] == 0, tg, rt["fixed"])
    assert np.abs(r3.mp_residual(rt["z"], p, q)).max() <= 1e-14


def test_fixture_rows_are_the_references():
    fx = r3.make_fixture()
    assert json.loads(json.dumps(fx)) == KATS
    g = KATS["residual_rows"]
    assert len(g["z"]) == 40 and np.array_equal(r3.mp_residual(g["z"][:5], g["p"][:5], g["q"][:5]), np.array(g["mp"][:5]))
    assert np.abs(r3.np_residual(g["z"], g["p"], g["q"]) - np.array(g["mp"])).max() <= 64 * lin_ref.EPS * 4
    rr = KATS["root_rows"]
    assert len(rr["z"]) == 48 and np.abs(r3.np_root(np.array(rr["dirs"]), np.array(rr["z"]), np.array(rr["fixed"])) - np.array(rr["mp"])).max() <= 64 * lin_ref.EPS * 4


def test_kats_against_the_restatement():
    k = KATS["kats"]
    assert len(k["cases"]) == 7 and k["norm_below"] == 1e-10
    assert [c["rpy"] for c in k["cases"]] == [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [-0.1, 0, 0], [0, -0.1, 0], [0, 0, -0.1]]
    for c in k["cases"]:
        assert np.linalg.norm(r3.np_residual([c["z"]], [c["p"]], [c["q"]])[0]) < k["norm_below"], c["rpy"]
        assert np.linalg.norm(r3.mp_residual([c["z"]], [c["p"]], [c["q"]])[0]) < k["norm_below"], c["rpy"]
        R_q = np.array(c["q"][3:]).reshape(3, 3).T                                # RotXYZ with one angle: the rotation about that axis
        ax = int(np.argmax(np.abs(c["rpy"]))) if any(c["rpy"]) else 0
        assert abs(R_q[ax, ax] - 1.0) <= 1e-15 and abs(np.trace(R_q) - (1 + 2 * math.cos(max(np.abs(c["rpy"]))))) <= 1e-15


def test_restatement_rows_land_on_roots_and_keep_the_translation():
    import oracle as ro
    N = 24
    rng = np.random.default_rng(4)
    poses = lambda: np.concatenate([rng.uniform(-40, 40, (3, N)), rng.standard_normal((3, N)) * 0.5])
    oo = ro.make_opts(N=N, solver=1, seed=5)
    fx, tg = poses(), poses()
    for d in (0, 1):
        out, st, z = r3.rot_row(oo, d, [0.3, -0.2, 0.5], COV, fx, tg, 7, r3.NEWTON)
        assert not st.any() and np.array_equal(out[:3], tg[:3]) and not np.array_equal(out[3:], tg[3:])
        r = r3.mp_residual(z, fx.T, out.T) if d == 0 else r3.mp_residual(z, out.T, fx.T)
        assert np.abs(r).max() <= 1e-13
    out, st, _ = r3.rot_row(oo, 0, [0.0, 0.0, 4.0], COV * 1e-6, fx, tg, 7, r3.NEWTON)
    assert st.all()                                                               # |z| >= pi: the functor has no zero


# ------------------------------------------------------------------ factor class, coverage, packing
def test_constructor_coverage_and_validation():
    f = R.Pose3Pose3Rotation(R.MvNormal([0.1, 0.2, 0.3], 0.1 * np.eye(3)))
    assert f.partial == (4, 5, 6) and f.variable_types == (R.Pose3, R.Pose3) and not f.is_prior
    assert R.Pose3Pose3Rotation in PARTIAL3_FACTORS
    assert partial_coverage(f, 0) == (3, 4, 5) and partial_coverage(R.Pose3Pose3Rotation, 1) == (3, 4, 5)
    with pytest.raises(ValueError):
        R.Pose3Pose3Rotation(R.MvNormal(np.zeros(6), np.eye(6)))
    with pytest.raises(TypeError):
        R.Pose3Pose3Rotation(R.Normal(0.0, 1.0))


def test_pack_unpack_roundtrip():
    pk = KATS["packing"]
    f = R.Pose3Pose3Rotation(R.MvNormal(pk["mu"], np.array(pk["cov"])))         # test/testpackingconverters.jl:256-264
    d = R.pack_factor(f)
    assert d["fnctype"] == "Pose3Pose3Rotation" and set(d) == {"fnctype", "Z"}   # PackedPose3Pose3Rotation: Z
    f2 = R.unpack_factor(d)
    assert type(f2) is R.Pose3Pose3Rotation and np.array_equal(f2.Z.mu, f.Z.mu) and np.array_equal(f2.Z.cov, f.Z.cov) and f2.partial == f.partial
    p = serialization.packFactor(f)
    assert set(p) == {"Z"}
    f3 = serialization.unpackFactor("RoME.PackedPose3Pose3Rotation", p)
    assert type(f3) is R.Pose3Pose3Rotation and np.array_equal(f3.Z.mu, f.Z.mu) and np.array_equal(f3.Z.cov, f.Z.cov)


def _graph(N=16, xyy=False, zrp=False, rot=True, full_odometry=False):
    """x0 with a PriorPose3, x0 -> x1 by the chosen factors"""
    fg = R.initfg(N=N)
    fg.addVariable("x0", R.Pose3); fg.addVariable("x1", R.Pose3)
    fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.diag([0.1] * 3 + [0.01] * 3) ** 2)))
    if full_odometry:
        fg.addFactor(["x0", "x1"], R.Pose3Pose3(R.MvNormal(np.zeros(6), np.eye(6) * 0.01)))
    if xyy:
        fg.addFactor(["x0", "x1"], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, 0.5], np.diag([0.1, 0.1, 0.01]) ** 2)))
    if zrp:
        fg.addFactor(["x1"], R.PriorPose3ZRP(R.Normal(1.0, 0.1), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2)))
    if rot:
        fg.addFactor(["x0", "x1"], R.Pose3Pose3Rotation(R.MvNormal([0.0, 0.0, 0.5], COV)), nullhypo=0.25)
    return fg


def _zero_init(fg):
    for l, t in fg.variables.items():
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    return fg


def test_save_load_roundtrip():
    fg = _graph(xyy=True, zrp=True)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "fg.tar.gz")
        R.saveDFG(fg, p)
        fg2 = R.loadDFG(p)
    key = lambda g: sorted((tuple(l), tuple(f.Z.mu), tuple(f.Z.cov.ravel())) for _, l, f in g.factors if isinstance(f, R.Pose3Pose3Rotation))
    assert len(key(fg2)) == 1 and key(fg2) == key(fg)
    assert sorted(type(f).__name__ for _, _, f in fg2.factors) == sorted(type(f).__name__ for _, _, f in fg.factors)


def test_packed_table_and_family_record():
    """p3rot is the LAST family, on the upper half of zrp3's stream slot; a graph without the factor keeps its plan"""
    fg = _graph(xyy=True, zrp=True)
    pk = R.PackedGraph(fg)
    ix = pk.index
    ro_ = pk.p3rot
    assert ro_["F"] == 1 and list(ro_["var_from"]) == [ix["x0"]] and list(ro_["var_to"]) == [ix["x1"]] and list(ro_["nh"]) == [0.25]
    assert ro_["mu"].tolist() == [[0.0, 0.0, 0.5]] and ro_["cov"].shape == (1, 3, 3) and pk.has_partial3()
    assert R.PackedGraph(_graph(rot=False)).p3rot["F"] == 0 and not R.PackedGraph(_graph(rot=False)).has_partial3()
    assert R.PackedGraph(_graph()).has_partial3()
    assert R.PackedGraph.from_pose2_tables(8, 2, np.zeros((1, 3)), np.eye(3)[None], [0], [1]).p3rot["F"] == 0
    dg = R.DeviceGraph(_zero_init(fg), plan_only=True)
    dg0 = R.DeviceGraph(_zero_init(_graph(xyy=True, zrp=True, rot=False)), plan_only=True)
    assert dg.STREAM_P3ROT == (14 << 28) + (1 << 27) and (dg.STREAM_P3XYY, dg.STREAM_ZRP3) == (13 << 28, 14 << 28)
    assert dg.STREAM_ZRP3 < dg.STREAM_P3ROT < dg.STREAM_PARTIAL2
    o = R.make_opts(N=16, solver=1, stream_offset=1000)
    plan, plan0 = dg.conv_plan(o, sweep=3), dg0.conv_plan(o, sweep=3)
    assert plan[:-1] == plan0
    last = plan[-1]
    assert last["name"] == "p3rot" and last["entry"] == "rome_conv_pose3pose3rotation_dev" and last["n_conv"] == 2
    assert last["stream_offset"] == 1000 + (3 << 32) + dg.STREAM_P3ROT and last["vt_target"] == "Pose3" and last["cols"] == ["nh"]
    assert last["prop_lo"] == dg0.n_prop[R.Pose3] and dg.n_prop[R.Pose3] == dg0.n_prop[R.Pose3] + 2 and not last["fused"]
    assert dg.families(every=True)[-1] == "p3rot" and dg.families(every=True)[:-1] == dg0.families(every=True)
    rec = dg.family_table("p3rot")
    assert rec["rows4"].tolist() == [[0, 0, ix["x0"], ix["x1"]], [0, 1, ix["x1"], ix["x0"]]] and tuple(rec["L"].shape) == (1, 6)
    assert rec["nh"].tolist() == [0.25, 0.25] and dg.fams["p3rot"]["partial"] == (3, 4, 5)
    assert dg.has_partial3() and dg0.has_partial3() and R.DeviceGraph(_zero_init(_graph()), plan_only=True).has_partial3()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_recorded_conv_plans_are_unchanged(name):
    want = json.load(open(FIXTURE))[name]
    got = describe(build(name, plan_only=True)[1])
    assert got["plan"] == want["plan"] and got["families"] == want["families"] and got["n_prop"] == want["n_prop"]


def _tasks(dg):
    pt = dg.tasks[R.Pose3]["host"]
    rows = [pt["task_rows"][pt["task_ptr"][k]:pt["task_ptr"][k + 1]].tolist() for k in range(len(pt["task_var"]))]
    return list(zip(pt["task_var"].tolist(), pt["task_coord"].tolist(), rows, pt["task_joint"].tolist()))


def test_partial_tasks_rotation_alone():
    """rows of prop[Pose3]: 0 the PriorPose3 of x0, 1 the rotation row towards x1, 2 the one towards x0"""
    dg = R.DeviceGraph(_zero_init(_graph()), plan_only=True)
    assert dg._prop_cover[R.Pose3] == [None, (3, 4, 5), (3, 4, 5)]
    assert _tasks(dg) == [(0, 3, [2], 1), (0, 4, [2], 1), (0, 5, [2], 1), (1, 3, [1], 0), (1, 4, [1], 0), (1, 5, [1], 0)]
    pt = dg.tasks[R.Pose3]["host"]
    assert pt["full_ptr"].tolist() == [0, 1, 1] and pt["full_rows"].tolist() == [0] and dg.tasks[R.Pose3]["any_joint"]


def test_partial_tasks_three_partial_families_on_one_variable():
    """rows: 0 PriorPose3 (x0); 1, 2 XYYaw (towards x1, x0); 3 ZRP (x1); 4, 5 Rotation (towards x1, x0).  On x1 coordinates 3 and 4 are
    covered by ZRP and Rotation, coordinate 5 by XYYaw and Rotation"""
    dg = R.DeviceGraph(_zero_init(_graph(xyy=True, zrp=True)), plan_only=True)
    assert dg._prop_cover[R.Pose3] == [None, (0, 1, 5), (0, 1, 5), (2, 3, 4), (3, 4, 5), (3, 4, 5)]
    assert _tasks(dg) == [(0, 0, [2], 1), (0, 1, [2], 1), (0, 3, [5], 1), (0, 4, [5], 1), (0, 5, [2, 5], 1),
                          (1, 0, [1], 0), (1, 1, [1], 0), (1, 2, [3], 0), (1, 3, [3, 4], 0), (1, 4, [3, 4], 0), (1, 5, [1, 4], 0)]


def test_header_and_shim_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_residual_pose3pose3rotation", "rome_residual_pose3pose3rotation_pt", "rome_conv_pose3pose3rotation",
           "rome_conv_pose3pose3rotation_dev"}
    assert new <= declared and new <= set(R._lib.SIGNATURES) and declared == set(R._lib.SIGNATURES)
    jl = open(os.path.join(ROOT, "rome.jl_amd", "julia", "RoMEMI355Ext.jl")).read()
    assert all((":%s," % n) in jl for n in new)
    assert R._lib.SIGNATURES["rome_conv_pose3pose3rotation"] == R._lib.SIGNATURES["rome_conv_pose3pose3xyyaw"]
    assert R._lib.SIGNATURES["rome_residual_pose3pose3rotation_pt"] == R._lib.SIGNATURES["rome_residual_pose3pose3xyyaw_pt"]


# ------------------------------------------------------------------ refusals
def test_refusals_name_the_factor():
    name = "Pose3Pose3Rotation"
    fg = _zero_init(_graph(full_odometry=True))
    lbl = [fl for fl, _, f in fg.factors if isinstance(f, R.Pose3Pose3Rotation)][0]
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


def test_multihypo_over_the_factor_raises():
    fg = _graph()
    fg.addVariable("x2", R.Pose3)
    with pytest.raises((TypeError, ValueError)):
        fg.addFactor(["x0", "x1", "x2"], R.Pose3Pose3Rotation(R.MvNormal([0.0, 0.0, 0.5], COV)), multihypo=[1.0, 0.5, 0.5])


def test_nelder_mead_restatement_converges_on_the_gpu_test_inputs():
    """the restatement alone, on the belief-shaped inputs of tests/test_gpu_rotation3.py: every particle ends with status 0 on a zero of
    the functor (g_tol = 1e-8 on the spread of sum r^2 leaves |r| of order 1e-4; measured: median 5.1e-5, largest 1.8e-4)"""
    import test_gpu_rotation3 as T
    dirs, mu, cov, fixed, target, noise = T.nm_inputs()
    ref, rst, z = T.nm_restatement()
    own = np.stack([np.abs(r3.np_residual(z[c], *((fixed[c].T, ref[c].T) if dirs[c] == 0 else (ref[c].T, fixed[c].T)))).max(axis=1)
                    for c in range(4)])
    print("restatement: status set on %d, own |r| median %.3e, max %.3e" % (int(rst.sum()), np.median(own), own.max()))
    assert not rst.any() and own.max() < 1e-3 and np.array_equal(ref[:, :3], target[:, :3])
