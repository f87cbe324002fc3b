#!/usr/bin/env python3
"""Writes tests/golden/gibbs_bits.json: the sha256 of the output bytes of the multiscale Gibbs product (rome_product_gibbs_dev) on
every table of tests/gibbs_tables.py, from the library that is loaded (ROME_MI355_LIB selects another build).  Run on the GPU with
the library of the commit whose bits are to be kept; tests/test_gpu_gibbs.py asserts that they have not changed.  Per table it also
prints the share of samples within 1e-9 of the oracle (ro.product_msgibbs, on the CPU): a recording is kept only when every table
meets the bar of test_device_equals_oracle_sample_by_sample (> 0.995), and it exits non-zero otherwise.

    python scripts/gibbs_bits.py [out.json]"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ORACLE_BAR = 0.995


def outputs(names):
    """{table name: bel_out (V, D, N) float64 on the host}"""
    import numpy as np
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    import gibbs_tables as GT
    lib, ctx = _lib.load(), R.default_context()

    def dev(a, dt):
        return torch.as_tensor(np.array(a), dtype=dt, device="cuda")   # (a copy: the shared tables are read-only)

    out = {}
    for name in names:
        t = GT.table(name)
        D, N, V = t["D"], t["N"], len(t["ptr"]) - 1
        ptr, rows = dev(t["ptr"], torch.int32), dev(t["rows"], torch.int32)
        prop, bw, bel = dev(t["prop"], torch.float64), dev(t["bw"], torch.float64), dev(t["bel"], torch.float64)
        new = torch.full((V, D, N), float("nan"), dtype=torch.float64, device="cuda")
        o = R.make_opts(N=N, seed=t["seed"], stream_offset=t["stream_offset"])
        torch.cuda.synchronize()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.rome_product_gibbs_dev(ctx.handle, C.byref(o), D, V, ptr.data_ptr(), rows.data_ptr(), prop.data_ptr(), bw.data_ptr(),
                                              len(t["prop"]), bel.data_ptr(), new.data_ptr(), t["circ"], t["iters"], int(np.diff(t["ptr"]).max())),
                   ctx.handle)
        torch.cuda.synchronize()
        out[name] = new.cpu().numpy()
    return out


def hashes(names):
    return {name: hashlib.sha256(a.tobytes()).hexdigest() for name, a in outputs(names).items()}


def oracle_share(name, got):
    """share of the (variable, sample) pairs of `got` within 1e-9 of the oracle's"""
    import numpy as np
    import oracle as ro
    import gibbs_tables as GT
    t = GT.table(name)
    D, N = t["D"], t["N"]
    ref = ro.product_msgibbs(ro.make_opts(N=N, seed=t["seed"], stream_offset=t["stream_offset"]), D, t["ptr"], t["rows"], t["prop"], t["bw"],
                             t["bel"], t["circ"], t["iters"])
    DE = 3 if D == 6 else D
    d = got[:, :DE] - ref[:, :DE]
    for k in range(DE):
        if (t["circ"] >> k) & 1:
            d[:, k] = np.arctan2(np.sin(d[:, k]), np.cos(d[:, k]))
    same = np.abs(d).max(axis=1) < 1e-9
    if D == 6:
        same &= GT.rotation_angle(got[:, 3:].transpose(0, 2, 1), ref[:, 3:].transpose(0, 2, 1)) < 1e-9
    return float(same.mean())


def main():
    import gibbs_tables as GT
    from rome_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gibbs_bits.json")
    got = outputs(GT.names())
    low = []
    for name, a in got.items():
        share = oracle_share(name, a)
        print("%-24s %6d samples  %.5f within 1e-9 of the oracle" % (name, a.shape[0] * a.shape[2], share), flush=True)
        if not share > ORACLE_BAR:
            low.append(name)
    doc = {"what": "sha256 of the float64 bytes of bel_out (V, D, N) of rome_product_gibbs_dev per table of tests/gibbs_tables.py",
           "library_version": int(_lib.load().rome_version()), "sha256": {n: hashlib.sha256(a.tobytes()).hexdigest() for n, a in got.items()}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d hashes -> %s" % (len(doc["sha256"]), out))
    if low:
        sys.exit("below the oracle bar of %.3f, recording not to be kept: %s" % (ORACLE_BAR, ", ".join(low)))


if __name__ == "__main__":
    main()
