#!/usr/bin/env python3
"""`solveTree` as variable elimination in relative-factor algebra on an SE(3) graph (BASELINE configs[4]: the synthetic helix with loop
closures between adjacent turns): from the factors alone -- no init pass, no starting beliefs -- to the neighbourhood of the parametric
solution.  Prints the translation RMS of the belief means to `solveGraphParametric` of the same graph, beside that of the dead-reckoned
start.

    python examples/helix3d_tree.py [poses [particles [passes]]]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rome_jl_amd as R  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 200
N = int(sys.argv[2]) if len(sys.argv) > 2 else 64          # (Pose3 products take N <= 256)
passes = int(sys.argv[3]) if len(sys.argv) > 3 else 1


def rms(fg, xp):
    labels = list(fg.variables)
    mean, _ = R.belief_stats(np.stack([fg.getVal(l) for l in labels]))
    return float(np.sqrt(np.mean(np.sum((mean[:, :3] - np.array([xp[l][:3] for l in labels])) ** 2, axis=1))))


start = R.dead_reckon_init_pose3(R.synth_helix3d(P=P, N=N, seed=4), seed=1)
xp = R.solveGraphParametric(R.dead_reckon_init_pose3(R.synth_helix3d(P=P, N=N, seed=4), seed=1))
fg = R.synth_helix3d(P=P, N=N, seed=4)
t = time.perf_counter()
es = R.solveTree(fg, messages="elimination", passes=passes, seed=11)     # (messages="auto" keeps the clique form for a Pose3 graph)
tt = time.perf_counter() - t
st = es.stats()
print("%d Pose3, %d factors, N = %d: solveTree(messages=\"elimination\"), %d pass(es), %.2f s wall-clock (%d rounds, %d merges, %d compositions, "
      "%d launch steps)" % (len(fg.variables), len(fg.factors), N, passes, tt, st["rounds"], st["merges"], st["compositions"], st["launch_steps"]))
print("translation RMS to the parametric solution: elimination %.3f m, dead-reckoned start %.3f m" % (rms(fg, xp), rms(start, xp)))
