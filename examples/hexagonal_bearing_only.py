#!/usr/bin/env python3
"""Counterpart of the reference's examples/Hexagonal2D_BearingOnly_SLAM.jl: a robot drives two rounds of a hexagon (13 legs of 10 m,
turning π/3 after each) and sees ONE landmark by direction only -- a camera without depth.  From the corners x0, x6, x12 the landmark
lies at bearing atan(10, 20), one leg later (x1, x7, x13) at atan(10, 10) − π/3; no sighting carries a distance.  A single bearing
leaves the landmark anywhere on a ray; the product of the six rays puts it near (20, 10).

    python examples/hexagonal_bearing_only.py [--sweeps K] [--particles N]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import rome_jl_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=12)
ap.add_argument("--particles", type=int, default=100)
args = ap.parse_args()

LEGS, TRUTH = 13, (20.0, 10.0)
odo_cov = np.diag([0.1, 0.1, 0.1]) ** 2
fg = R.initfg(N=args.particles)
fg.addVariable("x0", R.Pose2)
fg.addFactor(["x0"], R.PriorPose2(R.MvNormal(np.zeros(3), odo_cov)))
for i in range(LEGS):
    fg.addVariable("x%d" % (i + 1), R.Pose2)
    fg.addFactor(["x%d" % i, "x%d" % (i + 1)], R.Pose2Pose2(R.MvNormal([10.0, 0.0, math.pi / 3], odo_cov)))
fg.addVariable("l1", R.Point2)
at_corner, one_leg_on = math.atan2(10, 20), math.atan2(10, 10) - math.pi / 3
for k in range(0, LEGS, 6):
    fg.addFactor(["x%d" % k, "l1"], R.Pose2Point2Bearing(R.Normal(at_corner, 0.05)))
    fg.addFactor(["x%d" % (k + 1), "l1"], R.Pose2Point2Bearing(R.Normal(one_leg_on, 0.05)))

dg = R.solveGraph(fg, n_sweeps=args.sweeps, seed=7)      # initAll, then K x (all convolutions, all products) on the GPU
mean2, _ = dg.belief_stats(R.Pose2)
for label, m in zip(dg.packed.labels[R.Pose2], mean2.cpu().numpy()):
    print("%-4s mean (%7.2f, %7.2f, %6.2f)" % (label, *m))
l1 = fg.getVal("l1")
m = l1.mean(axis=1)
print("l1 mean (%.3f, %.3f)  distance from (%g, %g): %.3f" % (m[0], m[1], *TRUTH, math.hypot(m[0] - TRUTH[0], m[1] - TRUTH[1])))
