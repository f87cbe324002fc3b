#!/usr/bin/env python3
"""Writes tests/golden/kde_bits.json: the sha256 of the output bytes of rome_kde_bandwidth_dev on every (mask, stopping rules) run of
every table of tests/kde_ref.py (all_tables; the runs Reference.runs lists, taken from the table's `masks` and `runs` fields so that
no CPU reference is built) and of rome_kde_max_dev on every table of all_max_tables, from the library that is loaded (ROME_MI355_LIB
selects another build).  Run on the GPU with the library of the commit whose bits are to be kept; tests/test_gpu_kde_shapes.py asserts
that they have not changed.

    python scripts/kde_bits.py [out.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def run_key(name, mask, tols):
    return "bandwidth %s mask=%s tols=%g,%g" % (name, bin(mask), tols[0], tols[1])


def hashes():
    """{"bandwidth <table> mask=.. tols=..": sha256 of bw (V, dim), "max ..." (the table name): sha256 of the max-density points (V, dim)}"""
    import numpy as np
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    import kde_ref as KR
    lib, ctx = _lib.load(), R.default_context()

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")

    def sha(t):
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    out = {}
    for name, make in KR.all_tables():
        t = make()
        V, dim, N = t["bel"].shape
        bel = dev(t["bel"])
        for mask in t["masks"]:
            for tols in t["runs"]:
                a = (0.0, 0.0) if tols == KR.DEFAULT_TOLS else tols               # 0 selects the reference's stopping rules
                bw = torch.full((V * dim,), float("nan"), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                _lib.check(lib.rome_kde_bandwidth_dev(ctx.handle, dim, V, N, bel.data_ptr(), mask, a[0], a[1], bw.data_ptr()), ctx.handle)
                ctx.synchronize()
                out[run_key(name, mask, tols)] = sha(bw)
    for name, make in KR.all_max_tables():
        t = make()
        V, dim, N = t["bel"].shape
        bel, bw = dev(t["bel"]), dev(t["bw"])
        mx = torch.full((V * dim,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.rome_kde_max_dev(ctx.handle, dim, V, N, bel.data_ptr(), bw.data_ptr(), t["G"], mx.data_ptr()), ctx.handle)
        ctx.synchronize()
        out[name] = sha(mx)
    return out


def main():
    from rome_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "kde_bits.json")
    doc = {"what": "sha256 of the float64 output bytes: bw (V, dim) of rome_kde_bandwidth_dev per table of tests/kde_ref.py and per "
                   "(mask, stopping rules) run of it, the max-density points (V, dim) of rome_kde_max_dev per table of all_max_tables",
           "library_version": int(_lib.load().rome_version()), "sha256": hashes()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d hashes -> %s" % (len(doc["sha256"]), out))


if __name__ == "__main__":
    main()
