#!/usr/bin/env python3
"""Launch times of DeviceGraph.deconv (k_deconv, both outputs) next to the convolution sweep of the same table, on the two headline
tables: the Pose2Pose2 family of Manhattan-3500 and the Pose3Pose3 family of the 10k-pose helix, N = 100.  Device events around windows
of back-to-back launches after a warm-up; per case the time and the fraction of the HBM roofline (8.0 TB/s peak) on the ALGORITHMIC
bytes -- deconvolution: (da + db + 2 dz) x 8 per particle pair; sweep: (df + dt) x 8 per proposal particle -- per-row constants aside.
Run under `rocprofv3 --kernel-trace --stats -- python scripts/deconv_trace.py` for the kernel-level rows (no counters in that run)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import rome_jl_amd as R

HBM_PEAK = 8.0e12
N = 100


def windows(fn, reps=200, n_windows=5, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return out


def case(name, fg, kind, vt):
    dg = R.DeviceGraph(fg)
    g = torch.Generator(device="cuda").manual_seed(1)
    b = dg.bel[vt]
    b.copy_(torch.randn(b.shape, generator=g, device="cuda", dtype=torch.float64))
    if vt.dim == 6:
        b[:, 3:] *= 0.3
    o = R.make_opts(N=N, solver=R.SOLVER_CLOSED_FORM, seed=5)
    rec = dg.fams[kind]
    F = len(dg.deconv_labels(kind))
    d = vt.dim
    pred, meas = dg.deconv(o, kind)
    prop = torch.empty((rec["n"], d, N), dtype=torch.float64, device="cuda")
    for label, fn, nbytes in (("deconv, pred + meas", lambda: dg.deconv(o, kind, pred, meas), F * N * (2 * d + 2 * d) * 8),
                              ("deconv, pred only", lambda: dg.deconv(o, kind, pred, False), F * N * (2 * d + d) * 8),
                              ("convolution sweep", lambda: dg._sweep(rec, o, prop), rec["n"] * N * (2 * d) * 8)):
        us = windows(fn)
        best = min(us)
        print("%-22s %-20s rows %6d  us/launch %s  bytes %.3e  HBM roofline fraction %.3f (at the fastest window)"
              % (name, label, F if "deconv" in label else rec["n"], " ".join("%.2f" % u for u in us), nbytes, nbytes / HBM_PEAK / (best * 1e-6)))


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    case("Manhattan-3500 p2p2", R.synth_manhattan(N=N), "p2p2", R.Pose2)
    case("helix-10k p3p3", R.synth_helix3d(P=10000, N=N), "p3p3", R.Pose3)
