#!/usr/bin/env python3
"""Writes tests/golden/packed_sweep_bits.json: the sha256 of the proposal bytes of the packed sweep on the tables of
tests/sweep_shapes.py (GOLDEN_CASES), from the library that is loaded (ROME_MI355_LIB selects another build).  Run on the GPU with the
library of the commit whose bits are to be kept; tests/test_gpu_packed_sweep_shapes.py asserts that they have not changed.

    python scripts/packed_sweep_bits.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    import sweep_shapes as S
    env = (torch, _lib, _lib.load(), R.Context(0))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "packed_sweep_bits.json")
    doc = {"what": "sha256 of the float64 proposal bytes (rows, dt, N) of the packed sweep; key = family, N, rows, solver (tests/sweep_shapes.py)",
           "library_version": int(env[2].rome_version()), "sha256": S.golden_hashes(env)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
