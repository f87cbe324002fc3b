#!/usr/bin/env python3
"""Sweep timings of the bearing-only kernels (PB<1> landmark -> pose, PB<0> pose -> landmark) next to the bearing-range kernels
(BR<1>, BR<0>) on tables of the MIT-graph shape (5978 rows, N = 100), CLOSED_FORM and GAUSS_NEWTON; run under
`rocprofv3 --kernel-trace --stats -- python scripts/bearing_factors.py` for the kernel-level rows."""
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


N, F = 100, 5978
rng = np.random.default_rng(1)
fg = R.initfg(N=N)
for k in range(F):
    fg.addVariable("x%d" % k, R.Pose2)
    fg.addVariable("l%d" % k, R.Point2)
for k in range(F):
    b, r = float(rng.uniform(-3, 3)), float(rng.uniform(5, 20))
    fg.addFactor(["x%d" % k, "l%d" % k], R.Pose2Point2BearingRange(R.Normal(b, 0.05), R.Normal(r, 0.3)))
    fg.addFactor(["x%d" % k, "l%d" % k], R.Pose2Point2Bearing(R.Normal(b, 0.05)))
for k in range(F):
    c = rng.uniform(-100, 100, (2, 1))
    fg.initVariable("x%d" % k, np.vstack([c + rng.standard_normal((2, N)), rng.uniform(-3, 3) + 0.1 * rng.standard_normal((1, N))]))
    fg.initVariable("l%d" % k, c + rng.uniform(-15, 15, (2, 1)) + rng.standard_normal((2, N)))
dg = R.DeviceGraph(fg)
dg.upload_beliefs(fg)
out3 = torch.empty((F, 3, N), dtype=torch.float64, device="cuda")
out2 = torch.empty((F, 2, N), dtype=torch.float64, device="cuda")
for name, sv in (("closed_form", 0), ("gauss_newton", 3)):
    o = R.make_opts(N=N, solver=sv)
    for label, fn in (("BR<1> bearing-range -> pose", lambda: dg.sweep_bearingrange(o, 1, out=out3)),
                      ("PB<1> bearing-only  -> pose", lambda: dg.sweep_pose2point2bearing(o, 1, out=out3)),
                      ("BR<0> bearing-range -> landmark", lambda: dg.sweep_bearingrange(o, 0, out=out2)),
                      ("PB<0> bearing-only  -> landmark", lambda: dg.sweep_pose2point2bearing(o, 0, out=out2))):
        ms = timeit(fn, 20)
        print("%-32s %6d rows %-12s %9.4f ms/sweep  %.3e conv/s" % (label, F, name, ms, F / ms * 1e3))
