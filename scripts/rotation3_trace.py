#!/usr/bin/env python3
"""Sweep timings of the Pose3Pose3Rotation kernel (P3ROT) next to Pose3Pose3 (P3P3) and Pose3Pose3XYYaw (P3XYY) on the wave-per-row
kernel k_conv: 10000 rows of N = 100 each, CLOSED_FORM, in the manner of scripts/partial_pose3_trace.py.  With a given noise array
every family runs k_conv<., 0, 2, false> (P3P3 would otherwise take the packed sweep); the two partial families also run their plain
tables (k_conv<., 0, 2, true>, in-kernel Philox).  Run under `rocprofv3 --kernel-trace --stats -- python scripts/rotation3_trace.py`
for the kernel-level rows."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rome_jl_amd as R


def timeit(fn, reps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); one = max(time.perf_counter() - t0, 1e-6)
    for _ in range(min(2000, int(0.1 / one))):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


N, V = 100, 10000
rng = np.random.default_rng(1)
fg = R.initfg(N=N)
for k in range(V):
    fg.addVariable("x%d" % k, R.Pose3)
full = np.diag([0.1] * 3 + [0.01] * 3) ** 2
for k in range(0, V, 2):      # V/2 factors of each relative family = V rows
    fg.addFactor(["x%d" % k, "x%d" % (k + 1)], R.Pose3Pose3(R.MvNormal([10.0, 0, 0, 0, 0, math.pi / 2], full)))
    fg.addFactor(["x%d" % k, "x%d" % (k + 1)], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, math.pi / 2], np.diag([0.1, 0.1, 0.01]) ** 2)))
    fg.addFactor(["x%d" % k, "x%d" % (k + 1)], R.Pose3Pose3Rotation(R.MvNormal([0.0, 0.0, math.pi / 2], np.diag([0.01, 0.01, 0.01]) ** 2)))
centre = np.concatenate([rng.uniform(-100, 100, (V, 3)), rng.uniform(-0.3, 0.3, (V, 2)), rng.uniform(-3, 3, (V, 1))], axis=1)
for k in range(V):
    fg.initVariable("x%d" % k, centre[k][:, None] + rng.standard_normal((6, N)) * np.array([[0.5]] * 3 + [[0.05]] * 3))
dg = R.DeviceGraph(fg)
dg.upload_beliefs(fg)
out = torch.empty((V, 6, N), dtype=torch.float64, device="cuda")
noise6 = torch.randn((V, 6, N), dtype=torch.float64, device="cuda")
noise3 = torch.randn((V, 3, N), dtype=torch.float64, device="cuda")
o = R.make_opts(N=N, solver=0)
for label, fn in (("P3P3  Pose3Pose3, given noise", lambda: dg._sweep(dg.fams["p3p3"], o, out, noise6)),
                  ("P3XYY Pose3Pose3XYYaw, given noise", lambda: dg.sweep_pose3pose3xyyaw(o, out=out, noise=noise3)),
                  ("P3ROT Pose3Pose3Rotation, given noise", lambda: dg.sweep_pose3pose3rotation(o, out=out, noise=noise3)),
                  ("P3XYY Pose3Pose3XYYaw, in-kernel noise", lambda: dg.sweep_pose3pose3xyyaw(o, out=out)),
                  ("P3ROT Pose3Pose3Rotation, in-kernel noise", lambda: dg.sweep_pose3pose3rotation(o, out=out))):
    ms = timeit(fn, 20)
    print("%-42s %6d rows closed_form %9.4f ms/sweep  %.3e conv/s" % (label, V, ms, V / ms * 1e3))
