#!/usr/bin/env python3
"""Sweep timings of the range-only factor kernels (Point2Point2Range both directions, Pose2Point2Range dir 0 / dir 1) on ~10^4 rows of
N = 100, every solver; run under `rocprofv3 --kernel-trace --stats -- python scripts/range_factors.py` for the kernel-level rows.
Algorithmic bytes per particle (in-kernel RNG): fixed point / pose + the start point + the proposal written."""
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


N, F = 100, 5000
rng = np.random.default_rng(1)
fg = R.initfg(N=N)
for k in range(F + 1):
    fg.addVariable("l%d" % k, R.Point2)
for k in range(F):
    fg.addVariable("x%d" % k, R.Pose2)
for k in range(F):
    fg.addFactor(["l%d" % k, "l%d" % (k + 1)], R.Point2Point2Range(R.Normal(float(rng.uniform(5, 20)), 0.3)))
    fg.addFactor(["x%d" % k, "l%d" % k], R.Pose2Point2Range(R.Normal(float(rng.uniform(5, 20)), 0.3)))
for k in range(F + 1):
    fg.initVariable("l%d" % k, rng.uniform(-100, 100, (2, 1)) + rng.standard_normal((2, N)))
for k in range(F):
    fg.initVariable("x%d" % k, np.vstack([rng.uniform(-100, 100, (2, 1)) + rng.standard_normal((2, N)), rng.uniform(-3, 3) + 0.1 * rng.standard_normal((1, N))]))
dg = R.DeviceGraph(fg)
dg.upload_beliefs(fg)
Cr = dg.tab["p2rng"]["C"]
out2 = torch.empty((Cr, 2, N), dtype=torch.float64, device="cuda")
outq0 = torch.empty((F, 2, N), dtype=torch.float64, device="cuda")
outq1 = torch.empty((F, 3, N), dtype=torch.float64, device="cuda")
HBM = 8000.0   # GB/s
for name, sv in (("closed_form", 0), ("newton", 1), ("gauss_newton", 3), ("nelder_mead", 2)):
    reps = 3 if name == "nelder_mead" else 20
    o = R.make_opts(N=N, solver=sv)
    for label, rows, bpp, fn in (("Point2Point2Range", Cr, 48, lambda: dg.sweep_point2point2range(o, out=out2)),
                                 ("Pose2Point2Range dir 0", F, 56, lambda: dg.sweep_pose2point2range(o, 0, out=outq0)),
                                 ("Pose2Point2Range dir 1", F, 64, lambda: dg.sweep_pose2point2range(o, 1, out=outq1))):
        ms = timeit(fn, reps)
        gbs = rows * N * bpp / ms / 1e6
        print("%-24s %6d rows %-12s %9.4f ms/sweep  %.3e conv/s  %7.1f GB/s algorithmic (%d B/particle) = %.3f of %.0f GB/s"
              % (label, rows, name, ms, rows / ms * 1e3, gbs, bpp, gbs / HBM, HBM))
