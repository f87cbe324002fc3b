#!/usr/bin/env python3
"""product_step on a 2000-pose chain of the shape of test/testPartialPose3.jl:455-501 (PriorPose3 on x0, a PriorPose3ZRP on every other
pose, a Pose3Pose3XYYaw between neighbours), N = 100, with partial_product "off" or "coordinate" (argv[1]).  One conv_step fills the
proposals, then the product runs `reps` times.  Run under `rocprofv3 --kernel-trace --stats -- python scripts/partial_product_trace.py MODE`
for the kernel-level rows (profiles/partial_product_trace.md)."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rome_jl_amd as R

mode = sys.argv[1] if len(sys.argv) > 1 else "coordinate"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
N, V = 100, 2000
rng = np.random.default_rng(1)
fg = R.initfg(N=N)
for i in range(V):
    fg.addVariable("x%d" % i, R.Pose3)
fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.diag([0.1, 0.1, 0.1, 0.01, 0.01, 0.01]) ** 2)))
for i in range(1, V):
    fg.addFactor(["x%d" % i], R.PriorPose3ZRP(R.Normal(float(i % 7), 0.1), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2)))
for i in range(1, V):
    fg.addFactor(["x%d" % (i - 1), "x%d" % i], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, math.pi / 2], np.diag([0.1, 0.1, 0.01]) ** 2)))
pos = np.zeros((V, 6))
for i in range(1, V):          # the dead-reckoned square
    th = (i - 1) * math.pi / 2
    pos[i, :2] = pos[i - 1, :2] + 10.0 * np.array([math.cos(th), math.sin(th)])
    pos[i, 2], pos[i, 5] = i % 7, math.atan2(math.sin(i * math.pi / 2), math.cos(i * math.pi / 2))
for i in range(V):
    fg.initVariable("x%d" % i, pos[i][:, None] + rng.standard_normal((6, N)) * np.array([[0.3]] * 3 + [[0.02]] * 3))
dg = R.DeviceGraph(fg)
dg.upload_beliefs(fg)
o = R.make_opts(N=N, solver=1, seed=7)
dg.conv_step(o, 0)
for s in range(5):
    dg.product_step(o, s, partial_product=mode)
torch.cuda.synchronize()
t0 = time.perf_counter()
for s in range(reps):
    dg.product_step(o, 5 + s, partial_product=mode)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / reps * 1e3
tk = dg.tasks[R.Pose3]
print("partial_product=%-10s %d poses, %d proposal rows, %d tasks, N = %d: %.4f ms per product_step (wall, %d steps)"
      % (mode, V, dg.n_prop[R.Pose3], tk["T"] if mode == "coordinate" else 0, N, ms, reps))
assert torch.isfinite(dg.bel[R.Pose3]).all()
