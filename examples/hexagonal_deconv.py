#!/usr/bin/env python3
"""Per-factor consistency scores after a solve: the hexagon of examples/hexagonal_slam.py with a Pose2Pose2 loop closure x6 -> x0 (the
robot is back at the start, heading as it left).  For every odometry factor and for the closure it prints
    mmd( measurement the factor's two solved beliefs predict , samples of the measurement the factor carries )
(DeviceGraph.factor_mmd: approxDeconv + mmd on the device; the reference accepts a convolution at < 0.001, test/testBasicPose2Conv.jl:56):
  1. solved with the closure as driven;
  2. the closure's measurement replaced by a wrong one -- 4 m off and turned by 0.5 rad -- and scored against the beliefs of 1.: the
     wrong factor stands out by orders of magnitude (how a candidate closure is checked before it is trusted);
  3. solved again WITH the wrong closure: a confident wrong factor bends the chain to itself, and its own score falls back among the
     others (the score judges a factor against beliefs it has not yet shaped).

    python examples/hexagonal_deconv.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import rome_jl_amd as R  # noqa: E402

OPTS = R.make_opts(N=100, solver=R.SOLVER_NEWTON, seed=7)


def graph(closure_mu, beliefs=None):
    """the hexagon with its closure; beliefs: {label: (dim, N)} to start from, None = dead reckoning"""
    fg = R.generateGraph_Hexagonal(N=100)
    closure = fg.addFactor(["x6", "x0"], R.Pose2Pose2(R.MvNormal(closure_mu, np.diag([0.1, 0.1, 0.1]) ** 2)))
    if beliefs is None:
        R.dead_reckon_init(fg, seed=1)
        fg.initVariable("l1", np.array([[20.0], [0.0]]) + np.random.default_rng(0).standard_normal((2, 100)))
    else:
        for label, pts in beliefs.items():
            fg.initVariable(label, pts)
    dg = R.DeviceGraph(fg)
    dg.upload_beliefs(fg)
    return fg, dg, closure


def report(title, dg, closure):
    s = dict(zip(dg.deconv_labels("p2p2"), dg.factor_mmd(OPTS, "p2p2").cpu().numpy()))
    print(title)
    for label, v in s.items():
        print("  %-8s %-12s mmd(pred, meas) = %.3e" % (label, "loop closure" if label == closure else "odometry", v))
    print("  closure / largest odometry score: %.2f" % (s[closure] / max(v for l, v in s.items() if l != closure)))


WRONG = [4.0, 0.0, 0.5]
fg, dg, closure = graph([0.0, 0.0, 0.0])
dg.solve(OPTS, n_sweeps=12)
report("1. solved with the closure as driven, x6 -> x0 = (0, 0, 0)", dg, closure)
dg.download_beliefs(fg)
_, dg2, closure2 = graph(WRONG, beliefs={l: fg.getVal(l) for l in fg.ls()})
report("2. the closure replaced by a wrong one, (4, 0, 0.5), scored against the beliefs of 1.", dg2, closure2)
dg2.solve(OPTS, n_sweeps=12)
report("3. solved again with the wrong closure: the chain bends to it", dg2, closure2)
