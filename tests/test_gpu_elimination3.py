"""`solveTree(messages="elimination")` on Pose3 graphs, on the device: ROME_BLOCKOP_COMPOSE on Pose3 blocks and ROME_BLOCKOP_ANCHOR_MEAN
against the float64 and mpmath restatements of tests/elim3_ref.py (bounds: the rule of tests/test_elimination3_host.py, measured on the
CPU), the sampled-measurement Pose3Pose3 rows (`p3p3_meas`) against the oracle convolution, the whole solve against the oracle
restatement of the same schedule, and the solve itself against the parametric solution of the helix."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import rome_jl_amd as R   # noqa: E402
import oracle as ro   # noqa: E402
from rome_jl_amd import _lib   # noqa: E402
from rome_jl_amd.clique import DeviceStore, SampledPose3Pose3   # noqa: E402
from rome_jl_amd.elimination import RelativeEliminationSolver   # noqa: E402
from rome_jl_amd.graph import FactorGraph   # noqa: E402
from rome_jl_amd.tree import BlockOpPlan, LevelSpec, TreeLevelPlan   # noqa: E402
from dist_standin import OracleTreeBlockOp, OracleTreeStore   # noqa: E402
import elim3_ref as E3   # noqa: E402


# N: the wave and block edges (257 takes the strided loop round a second time; block operations carry no 256 cap)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 256, 257])
def test_pose3_block_operations_against_the_restatement_and_mp(N):
    ref = E3.reference(N)
    cs, an = ref["cases"], ref["anchors"]
    fg = R.initfg(N)
    for j, c in enumerate(cs):
        for pre in "abder":
            fg.addVariable("%s%d" % (pre, j), R.Pose3)
        fg.initVariable("a%d" % j, c["A"]); fg.initVariable("b%d" % j, c["B"])
    for j, a in enumerate(an):
        fg.addVariable("s%d" % j, R.Pose3); fg.addVariable("m%d" % j, R.Pose3); fg.addVariable("o%d" % j, R.Pose3)
        fg.initVariable("s%d" % j, a)
    rng = np.random.default_rng(7)
    for l, vt in (("p", R.Pose2), ("l", R.Point2)):      # ANCHOR_MEAN on Pose2 / Point2 is ANCHOR
        for k in range(3):
            fg.addVariable("%s%d" % (l, k), vt)
        fg.initVariable(l + "0", np.array([[3.0], [-2.0], [3.1]])[:vt.dim] + 0.4 * rng.standard_normal((vt.dim, N)))
    dev, orc = DeviceStore(fg), OracleTreeStore(R, fg)
    orc.upload(fg)
    ent = [("a%d" % j, "b%d" % j, "d%d" % j, c["flags"][0], c["flags"][1]) for j, c in enumerate(cs)]
    BlockOpPlan(dev, "compose", ent).run()                                                              # params = NULL
    BlockOpPlan(dev, "compose", [("a%d" % j, "b%d" % j, "e%d" % j) + e[3:] + c["prm"] for j, (e, c) in enumerate(zip(ent, cs))]).run()
    plain = [dev.get("d%d" % j) for j in range(len(cs))]
    infl = [dev.get("e%d" % j) for j in range(len(cs))]
    f0 = E3.check_blocks(plain, ref, "compose", inflated=False)
    f1 = E3.check_blocks(infl, ref, "compose with params")
    print("ELIM3 gpu N=%d compose (units of the bound): plain %s, with params %s" % (N, f0, f1))
    for j, c in enumerate(cs):                      # params exactly (1, 1): the plain composition, bit for bit
        if c["prm"] == (1.0, 1.0):
            assert np.array_equal(plain[j], infl[j]), j
    for j in range(len(cs)):                        # the inputs were not touched
        assert np.array_equal(dev.get("a%d" % j), cs[j]["A"]) and np.array_equal(dev.get("b%d" % j), cs[j]["B"])
    # a^-1 (+) b composed back onto a returns b: two operations, each within the bound of its exact result, and the second maps the first's
    # deviation one to one (a rotation of the translation error, a product of unit quaternions) -> twice the bound
    back = [j for j, c in enumerate(cs) if c["flags"] == (True, False) and c["kind"] in ("random", "edge", "axis") and not ref["zone"][j].any()]
    assert len(back) >= 4
    BlockOpPlan(dev, "compose", [("a%d" % j, "d%d" % j, "r%d" % j, False, False) for j in back]).run()
    for j in back:
        et, er = E3.np_distance(dev.get("r%d" % j), cs[j]["B"])
        assert et.max() <= 2 * ref["bound"]["compose_t"] * ref["tscale"][j] and er.max() <= 2 * ref["bound"]["compose_r"], (j, et.max(), er.max())
    # the mean anchor (tight and wide belief) in one plan with Pose2 / Point2 entries; ANCHOR on the same blocks keeps particle 0's rotation
    BlockOpPlan(dev, "anchor_mean", [("p0", "p2"), ("s0", "m0"), ("l0", "l2"), ("s1", "m1")]).run()
    BlockOpPlan(dev, "anchor", [("p0", "p1"), ("l0", "l1"), ("s0", "o0"), ("s1", "o1")]).run()
    fa = E3.check_anchors([dev.get("m0"), dev.get("m1")], ref, "anchor_mean")
    print("ELIM3 gpu N=%d anchor_mean (units of the bound): %s" % (N, fa))
    assert np.array_equal(dev.get("p2"), dev.get("p1")) and np.array_equal(dev.get("l2"), dev.get("l1"))
    for j, a in enumerate(an):
        o = dev.get("o%d" % j)
        assert np.array_equal(o[3:], np.repeat(a[3:, :1], N, axis=1)) and np.array_equal(dev.get("s%d" % j), a)
    BlockOpPlan(dev, "anchor_mean", [("s0", "s0")]).run()     # in place
    assert np.array_equal(dev.get("s0"), dev.get("m0"))
    # COPY and MIX on Pose3 blocks
    steps = [("copy", [("d0", "r0"), ("e1", "r1")]), ("mix", [("a2", "b2", 3), ("a3", "b3", 1)])]
    for l in ("d0", "e1", "a2", "b2", "a3", "b3"):
        orc.vals[l] = dev.get(l)
    for op, e in steps:
        BlockOpPlan(dev, op, e).run(); OracleTreeBlockOp(orc, op, e).run()
    for l in ("r0", "r1", "b2", "b3"):
        assert np.array_equal(dev.get(l), orc.vals[l]), l


def _create(store, op, ty, a, b, d, prm=None):
    lib = _lib.load()
    PI = C.POINTER(C.c_int32)
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)     # noqa: E731
    ty, a, b, d = arr(ty), arr(a), arr(b), arr(d)
    p = None if prm is None else np.ascontiguousarray(prm, dtype=np.float64)
    h = C.c_void_p()
    rc = lib.rome_blockop_plan_create_ex(store.ctx.handle, store.handle, op, len(ty), ty.ctypes.data_as(PI), a.ctypes.data_as(PI),
                                         None if b is None else b.ctypes.data_as(PI), d.ctypes.data_as(PI),
                                         None if p is None else p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
    if rc == 0:
        lib.rome_blockop_plan_destroy(h)
    return rc


def test_pose3_block_operation_plans_refuse_invalid_arguments():
    fg = R.initfg(16)
    for k in range(4):
        fg.addVariable("x%d" % k, R.Pose2); fg.addVariable("q%d" % k, R.Pose3)
    st = DeviceStore(fg)
    COMPOSE, ANCHOR_MEAN, INV = 3, 5, _lib.ERR_INVALID_ARG
    assert BlockOpPlan.OPS["compose"] == COMPOSE and BlockOpPlan.OPS["anchor_mean"] == ANCHOR_MEAN
    assert _create(st, COMPOSE, [2, 2 | 0x100 | 0x200], [0, 0], [1, 1], [2, 3]) == 0                # all-Pose3: accepted
    assert _create(st, COMPOSE, [0, 0], [0, 0], [1, 1], [2, 3]) == 0                                # all-Pose2: as before
    assert _create(st, COMPOSE, [2, 2], [0, 0], [1, 1], [2, 3], prm=[1.3, 0.8, 1.0, 1.0]) == 0
    assert _create(st, ANCHOR_MEAN, [0, 2], [0, 0], None, [1, 1]) == 0
    assert _create(st, COMPOSE, [2, 0], [0, 0], [1, 1], [2, 2]) == INV                               # mixed types
    assert _create(st, COMPOSE, [0, 2], [0, 0], [1, 1], [2, 2]) == INV
    assert _create(st, COMPOSE, [2], [0], [1], [0]) == INV                                           # dst == a
    assert _create(st, COMPOSE, [2], [0], [1], [1]) == INV                                           # dst == b
    assert _create(st, COMPOSE, [2], [4], [1], [2]) == INV                                           # Pose3 indices out of range
    assert _create(st, COMPOSE, [2], [0], [4], [2]) == INV
    assert _create(st, COMPOSE, [2], [0], [1], [4]) == INV
    assert _create(st, COMPOSE, [2], [0], [-1], [2]) == INV
    assert _create(st, ANCHOR_MEAN, [2], [0], None, [4]) == INV
    assert _create(st, COMPOSE, [1], [0], [0], [0]) == INV                                           # Point2 has no composition
    assert _create(st, ANCHOR_MEAN, [2], [0], None, [1], prm=[1.0, 1.0]) == INV                       # params with a non-COMPOSE op
    assert _create(st, 0, [2], [0], None, [1], prm=[1.0, 1.0]) == INV
    assert _create(st, ANCHOR_MEAN, [2 | 0x100], [0], None, [1]) == INV                               # flags belong to COMPOSE / MIX
    assert _create(st, 6, [2], [0], None, [1]) == INV                                                 # past the last op


@pytest.mark.parametrize("N", [33, 64, 256])
def test_sampled_pose3pose3_rows_equal_the_oracle_convolution(N):
    """one SampledPose3Pose3 row in each direction over a store: the destination's single proposal IS its new belief (a product of one
    proposal is a copy) = the oracle convolution given the same samples.  Tolerances: tests/test_gpu_parity.py test_pose3pose3_vs_oracle."""
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(300 + N)
    sc = np.array([0.2, 0.2, 0.2, 0.05, 0.05, 0.05])[:, None]
    x = rng.standard_normal((6, N)) * sc + rng.standard_normal((6, 1)) * np.array([8, 8, 8, 0.8, 0.8, 0.8])[:, None]
    z = rng.standard_normal((6, N)) * sc + rng.standard_normal((6, 1)) * np.array([2, 2, 2, 0.5, 0.5, 0.5])[:, None]
    U = FactorGraph(N)
    for l in ("x", "z", "y", "w"):
        U.addVariable(l, R.Pose3)
    U.initVariable("x", x); U.initVariable("z", z)
    st = DeviceStore(U)
    L = FactorGraph(N)
    for l in ("x", "z", "y", "w"):
        L.addVariable(l, R.Pose3)
    for fl, labels in (("f0", ["x", "y"]), ("f1", ["w", "x"])):      # y = x (+) z;  w = x (-) z
        L.putFactor(fl, labels, SampledPose3Pose3("z"))
    spec = LevelSpec(L, [(["y"], [0]), (["w"], [0])], {"y": ["f0"], "w": ["f1"]}, [], 1)
    TreeLevelPlan(st, spec).run(R.make_opts(N=N, seed=5))
    out = np.stack([st.get("y"), st.get("w")])
    bel = np.stack([x, np.zeros((6, N)), np.zeros((6, N))])
    ref = ro.conv_pose3pose3(ro.make_opts(N=N, solver=1, seed=5), np.zeros((1, 6)), ro.cholesky_lower(np.eye(6))[None], bel, [0, 0], [1, 2], [0, 1],
                             factor=[0, 0], noise=np.stack([z, z]))
    near = np.linalg.norm(ref[:, 3:], axis=1) > np.pi - 1e-2
    ang = (Rot.from_rotvec(out[:, 3:].transpose(0, 2, 1).reshape(-1, 3)).inv() *
           Rot.from_rotvec(ref[:, 3:].transpose(0, 2, 1).reshape(-1, 3))).magnitude().reshape(near.shape)
    assert np.abs(out[:, :3] - ref[:, :3]).max() < 1e-9
    assert ang[~near].max() < 1e-9 and (not near.any() or ang[near].max() < 1e-6)
    assert np.array_equal(st.get("x"), x) and np.array_equal(st.get("z"), z)
    # the same composition through ROME_BLOCKOP_COMPOSE: the coordinates of a composed relative pose are what the row consumes
    E = E3.compose3(x, z)
    et, er = E3.np_distance(out[0], E)
    assert et.max() < 1e-9 and er.max() < 1e-9


def _diff3(a, b):
    """(6, N) blocks -> per-particle distance (max |Δt|, rotation angle) and the mean difference vector (Δt, Log(R_bᵀ R_a))"""
    ta, qa = E3.load3(a); tb, qb = E3.load3(b)
    d = np.concatenate([ta - tb, E3.q_log_snap(E3.q_mul(E3.q_conj(qb), qa))], axis=1)
    return np.maximum(np.abs(d[:, :3]).max(axis=1), np.sqrt((d[:, 3:] ** 2).sum(axis=1))), np.abs(d.mean(axis=0)).max()


def test_helix_elimination_equals_the_oracle_restatement():
    """120 poses with closures every 5th pose, N = 32, two structures, two pooled passes: merges, compositions, mean anchors, sampled rows,
    the pooling -- device == oracle restatement (criterion of tests/test_gpu_elimination.py / test_gpu_tree.py)"""
    fg = R.synth_helix3d(P=120, N=32, seed=4)
    dev = RelativeEliminationSolver(fg, structures=2)
    orc = RelativeEliminationSolver(fg, backend=E3.Elim3Backend(R), structures=2)
    st = dev.stats()
    assert st["merges"] > 0 and st["compositions"] > 100, st
    worst = []
    for ps in range(2):
        o = R.make_opts(N=fg.N, seed=71 + ps)
        dev.solve(o); orc.solve(o)
        fr, dm = [], []
        for l in fg.variables:
            d, m = _diff3(dev.store.get(l), orc.store.get(l))
            fr.append(np.mean(d < 1e-6)); dm.append(m)
        worst.append((float(np.mean(fr)), float(np.max(dm))))
    print("ELIM3 gpu helix P=120 N=32 seed 4 / 71: (fraction within 1e-6, worst |mean difference|) per pass %s; %s" % (worst, st))
    for frac, dmean in worst:
        assert frac > 0.9 and dmean < 1e-3, worst


def _rms_to(fg, xp):
    m, _ = R.belief_stats(np.stack([fg.getVal(l) for l in fg.variables]))
    return float(np.sqrt(np.mean(np.sum((m[:, :3] - np.array([xp[l][:3] for l in fg.variables])) ** 2, axis=1))))


def test_helix_elimination_solves():
    """synth_helix3d(P=200, N=64): translation RMS of the belief means to solveGraphParametric of the same graph -- the elimination form from
    the factors alone is closer than the dead-reckoned start, and closer than the clique form ("marginal") started from that init"""
    mk = lambda: R.synth_helix3d(P=200, N=64, seed=4)     # noqa: E731
    xp = R.solveGraphParametric(R.dead_reckon_init_pose3(mk(), seed=1))
    init = R.dead_reckon_init_pose3(mk(), seed=1)
    r_init = _rms_to(init, xp)
    marg = R.dead_reckon_init_pose3(mk(), seed=1)
    ts = R.solveTree(marg, messages="marginal", seed=5)
    r_marg = _rms_to(marg, xp)
    fg = mk()
    es = R.solveTree(fg, messages="elimination", seed=5)
    r_elim = _rms_to(fg, xp)
    print("ELIM3 gpu helix P=200 N=64: translation RMS to the parametric solution: elimination %.4f m, dead-reckoned init %.4f m, marginal tree "
          "solve from that init %.4f m; %s" % (r_elim, r_init, r_marg, es.stats()))
    assert ts.messages == "marginal" and es.messages == "elimination" and all(fg.isInitialized(l) for l in fg.variables)
    assert r_elim < r_init and r_elim < r_marg, (r_elim, r_init, r_marg)


def test_solve_tree_auto_still_takes_the_marginal_form_for_a_pose3_graph():
    fg = R.synth_helix3d(P=30, N=32, seed=4)
    R.dead_reckon_init_pose3(fg, seed=2)
    ts = R.solveTree(fg, seed=5)
    assert ts.messages == "marginal"
    assert not RelativeEliminationSolver.covers(fg) and RelativeEliminationSolver.covers(fg, pose3=True)
