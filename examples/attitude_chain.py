#!/usr/bin/env python3
"""A short chain of Pose3 variables measured only by partial factors (RoME src/factors/PartialPose3.jl): planar odometry with heading
(`Pose3Pose3XYYaw`, coordinates x, y, yaw), the relative attitude between neighbours as a gyro / AHRS integration gives it
(`Pose3Pose3Rotation`, the three rotation coordinates) and a depth + roll / pitch sensor on every pose (`PriorPose3ZRP`).  The vehicle
drives a quarter turn to the left per leg while descending one metre.  Solved with the partial-aware product: every coordinate is the
product of the proposals that cover it.

    python examples/attitude_chain.py [--poses K] [--sweeps S] [--particles N]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import rome_jl_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=5)
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--particles", type=int, default=100)
args = ap.parse_args()

fg = R.initfg(N=args.particles)
fg.addVariable("x0", R.Pose3)
fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.diag([0.1, 0.1, 0.1, 0.01, 0.01, 0.01]) ** 2)))
for i in range(1, args.poses):
    fg.addVariable("x%d" % i, R.Pose3)
    fg.addFactor(["x%d" % (i - 1), "x%d" % i], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, math.pi / 2], np.diag([0.1, 0.1, 0.01]) ** 2)))
    fg.addFactor(["x%d" % (i - 1), "x%d" % i], R.Pose3Pose3Rotation(R.MvNormal([0.0, 0.0, math.pi / 2], np.diag([0.01, 0.01, 0.01]) ** 2)))
    fg.addFactor(["x%d" % i], R.PriorPose3ZRP(R.Normal(-float(i), 0.1), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2)))

dg = R.solveGraph(fg, n_sweeps=args.sweeps, seed=7, partial_product="coordinate")
mean3, _ = dg.belief_stats(R.Pose3)
for label, m in zip(dg.packed.labels[R.Pose3], mean3.cpu().numpy()):
    print("%-4s mean t (%7.2f, %7.2f, %6.2f)  w (%6.3f, %6.3f, %6.3f)" % (label, *m))
