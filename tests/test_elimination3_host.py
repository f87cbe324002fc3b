"""Pose3 elimination, host side (no GPU): the float64 restatement of ROME_BLOCKOP_COMPOSE on Pose3 blocks / ROME_BLOCKOP_ANCHOR_MEAN
(tests/elim3_ref.py) against its mpmath restatement, and the structure of `RelativeEliminationSolver` on a Pose3 graph with the oracle
backend.

Cases (elim3_ref.cases): the SE(3) angle edges of tests/conv_ref.py (P3_MAGS: 0, tiny, mid-range, just below π, the two magnitudes inside
the snap zone, 4.0) as the angle of the COMPOSITION about each particle's own axis; common-axis compositions 2 + 2 > π (the w >= 0
representative); random rotations; beliefs composed with and without inflation; all four invert combinations; translation scales 1 and 100.
Rotations are compared as group elements (the angle of R_refᵀ R) everywhere; inside the snap zone (2 q_w² <= √eps, 2 of 48 cases: 4.2 %,
under the 5 % cap of tests/test_gpu_device_math.py) by the snap rule instead (|ω| = π within 4 ulp, the axis within the bound).  No case
lies within ZONE_MARGIN of the zone's edge.

Bound rule (tests/test_gpu_device_math.py), per output block: bound = max(8 dev, 64 ulp) x scale, dev = the float64 restatement's
deviation from mp measured HERE, scale = max(1, largest |translation| among the block's inputs and outputs) for translations, 1 for
rotation angles.  Measured dev (N = 65, units of eps = 2^-52): compose translation 1.31, rotation 3.12; inflated translation 0.59,
rotation 2.41; mean anchor translation 0.51, rotation 3.13 -- every bound is the 64 ulp floor."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rome_jl_amd as R   # noqa: E402
from rome_jl_amd.elimination import RelativeEliminationSolver   # noqa: E402
import conv_ref as CR   # noqa: E402
import elim3_ref as E3   # noqa: E402

N_HOST = 65


def test_float64_restatement_against_mpmath():
    ref = E3.reference(N_HOST)
    eps = 2.0 ** -52
    print("ELIM3 host dev (eps): " + ", ".join("%s %.2f" % (k, v / eps) for k, v in ref["dev"].items()))
    zone = np.concatenate(ref["zone"])
    n_zone_cases = sum(bool(z.any()) for z in ref["zone"])
    assert n_zone_cases == 2 and all(z.all() or not z.any() for z in ref["zone"])
    assert 0 < zone.mean() < 0.05, zone.mean()
    assert ref["margin"] >= CR.ZONE_MARGIN, ref["margin"]
    assert all(b == 64.0 * eps for b in ref["bound"].values()), ref["dev"]      # the figures of the header comment
    flags = {c["flags"] for c in ref["cases"]}
    assert len(flags) == 4 and {c["scale"] for c in ref["cases"]} == {1.0, 100.0}
    for kind in ("edge", "axis", "random", "belief"):
        assert {c["flags"] for c in ref["cases"] if c["kind"] == kind} == flags, kind
    # the reference against itself: the float64 outputs satisfy the bound against mp (what the device is asked)
    E3.check_blocks(ref["out"], ref, "float64")
    E3.check_anchors(ref["anchor"], ref, "float64")


def test_restatement_properties():
    """the w >= 0 representative past π; exact (1, 1) inflation; inflation keeps the mean and scales the spread; a^-1 (+) b composed back
    onto a returns b; the mean anchor of N copies is the point"""
    ref = E3.reference(N_HOST)
    for c, d, o in zip(ref["cases"], ref["D"], ref["out"]):
        th = np.sqrt((d[3:] ** 2).sum(0))
        assert (th <= math.pi + 4 * CR.ULP_PI).all()
        if c["kind"] == "axis":
            assert np.allclose(th, 2 * math.pi - 4.0, atol=1e-12)
        if c["prm"] == (1.0, 1.0):
            assert np.array_equal(d, o)
        else:
            (tm0, qm0), (tm1, qm1) = E3.mean3(d), E3.mean3(o)
            # (the translation mean is kept to rounding; the rotation mean is taken in the chart at particle 0 and the deviations are
            #  scaled in the chart at the mean: the two agree to second order in the spread, 0.05 rad here)
            assert np.abs(tm0 - tm1).max() <= 64 * 2.0 ** -52 * c["scale"] * 8 and CR.q_angle(CR.q_mul(CR.q_conj(qm0), qm1)) < 0.05 ** 2
            assert np.allclose(o[:3].std(1), c["prm"][0] * d[:3].std(1), rtol=1e-9)
    rng = np.random.default_rng(3)
    a = np.concatenate([5 * rng.standard_normal((3, 40)), (CR._unit(rng, (40,)) * rng.uniform(0, 3, (40, 1))).T])
    b = np.concatenate([5 * rng.standard_normal((3, 40)), (CR._unit(rng, (40,)) * rng.uniform(0, 3, (40, 1))).T])
    back = E3.compose3(a, E3.compose3(a, b, True, False))
    et, er = E3.np_distance(back, b)
    assert et.max() < 1e-13 and er.max() < 1e-14
    pt = np.repeat(a[:, :1], 40, axis=1)
    et, er = E3.np_distance(E3.anchor_mean3(pt), pt)
    assert et.max() < 1e-14 and er.max() < 1e-15


def test_pose3_solver_constructs_and_runs_one_pass_on_the_oracle_backend():
    fg = R.synth_helix3d(P=40, N=32, seed=4)
    es = RelativeEliminationSolver(fg, backend=E3.Elim3Backend(R))
    es.solve(R.make_opts(N=32, seed=9))
    st = es.stats()
    assert st["compositions"] > 0 and st["merges"] > 0, st
    assert any(k == "anchor_mean" for k, _ in es.schedules[0]) and not any(k == "anchor" for k, _ in es.schedules[0])
    for l in fg.variables:
        b = es.store.get(l)
        assert b.shape == (6, 32) and np.isfinite(b).all(), l
    m = np.array([es.store.get(l)[:3].mean(1) for l in fg.variables])
    gt = np.array([fg.ground_truth[l][:3] for l in fg.variables])
    print("ELIM3 host helix P=40 N=32: translation RMS of one oracle pass to the ground truth %.3f m; %s"
          % (np.sqrt(np.mean(np.sum((m - gt) ** 2, axis=1))), {k: st[k] for k in ("rounds", "merges", "compositions", "transports", "launch_steps")}))


def test_constructor_errors_and_the_unchanged_auto_predicate():
    fg = R.synth_helix3d(P=12, N=32, seed=4)
    assert RelativeEliminationSolver.covers(fg) is False and RelativeEliminationSolver.covers(fg, pose3=True) is True
    mixed = R.synth_helix3d(P=6, N=32, seed=4)
    mixed.addVariable("p0", R.Pose2)
    mixed.addFactor(["p0"], R.PriorPose2(R.MvNormal(np.zeros(3), np.eye(3) * 0.01)))
    with pytest.raises(TypeError):
        RelativeEliminationSolver(mixed, backend=E3.Elim3Backend(R))
    big = R.synth_helix3d(P=6, N=300, seed=4)
    with pytest.raises(ValueError, match="256"):
        RelativeEliminationSolver(big, backend=E3.Elim3Backend(R))
    p2 = R.generateGraph_Hexagonal(N=32)            # (a landmark: outside both scopes)
    with pytest.raises(TypeError):
        RelativeEliminationSolver(p2, backend=E3.Elim3Backend(R))
