#!/usr/bin/env python3
"""Writes tests/golden/product_bits.json: the sha256 of the output bytes of the importance product on every table of
tests/product_ref.py (all_tables) and of the belief statistics on every (D, N) of its SHAPE_N, from the library that is loaded
(ROME_MI355_LIB selects another build).  Run on the GPU with the library of the commit whose bits are to be kept;
tests/test_gpu_product.py asserts that they have not changed.

    python scripts/product_bits.py [out.json]"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def hashes(table_of=lambda name, make: make()):
    """{"product <table>": sha256 of bel_out (V, D, N), "stats D=.. N=..": sha256 of mean (V, D) then sdev (V, D)}; table_of lets a
    caller that already holds the tables hand them over"""
    import numpy as np
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    import product_ref as PR
    lib, ctx = _lib.load(), R.default_context()

    def dev(a, dt):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")

    out = {}
    for name, make in PR.all_tables():
        t = table_of(name, make)
        D, N, V = t["D"], t["N"], len(t["ptr"]) - 1
        ptr, rows, prop, bel = dev(t["ptr"], torch.int32), dev(t["rows"], torch.int32), dev(t["prop"], torch.float64), dev(t["bel"], torch.float64)
        new = torch.full((V * D * N,), float("nan"), dtype=torch.float64, device="cuda")
        o = R.make_opts(N=N, seed=t["seed"], stream_offset=t["stream_offset"])
        torch.cuda.synchronize()
        if t["bw"] is None:
            rc = lib.rome_product_dev(ctx.handle, C.byref(o), D, V, ptr.data_ptr(), rows.data_ptr(), prop.data_ptr(), bel.data_ptr(), new.data_ptr())
        else:
            bw = dev(t["bw"], torch.float64)
            rc = lib.rome_product_bw_dev(ctx.handle, C.byref(o), D, V, ptr.data_ptr(), rows.data_ptr(), prop.data_ptr(), bw.data_ptr(),
                                         bel.data_ptr(), new.data_ptr())
        _lib.check(rc, ctx.handle)
        ctx.synchronize()
        out["product " + name] = _sha(new)
    for D in PR.DIMS:
        for N in PR.SHAPE_N[D]:
            bel = dev(PR.stats_table(D, N), torch.float64)
            mean, sd = (torch.full((PR.STATS_V * D,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            _lib.check(lib.rome_belief_stats_dev(ctx.handle, D, PR.STATS_V, N, bel.data_ptr(), mean.data_ptr(), sd.data_ptr()), ctx.handle)
            ctx.synchronize()
            out["stats D=%d N=%d" % (D, N)] = _sha(mean, sd)
    return out


def main():
    from rome_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "product_bits.json")
    doc = {"what": "sha256 of the float64 output bytes: bel_out (V, D, N) of rome_product_dev / rome_product_bw_dev per table of "
                   "tests/product_ref.py, mean then sdev (V, D) of rome_belief_stats_dev per (D, N)",
           "library_version": int(_lib.load().rome_version()), "sha256": hashes()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d hashes -> %s" % (len(doc["sha256"]), out))


if __name__ == "__main__":
    main()
