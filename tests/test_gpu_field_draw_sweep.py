"""The kernels that draw Pose2 measurements through box_muller_field, at the smallest shapes at which the draw's plumbing can go wrong,
against tests/conv_ref.py's float64 root fed with the oracle's draws (ro.rng_normals) for the same seed and streams: np.array_equal.

Equality of bits with a NumPy root needs a table on which every operation after the draw is exact or a single rounding both sides
share: the Cholesky factors are float32 values (a draw has a 24-bit mantissa: every product L·ξ is exact, so the kernel's fused
multiply-adds round what NumPy's multiply-then-add rounds), every fixed heading is 0 (cos = 1, sin = 0 exactly: the rotation of the
measured translation is the identity), and the factor of the dir-1 rows has no heading noise and μ_θ = 0 (the returned heading, whose
frame turns the translation, is again 0).  Dir-0 and prior rows carry all three draws of both particles of a pair into the output.

Six rows: dir 0, dir 1, prior, dir 0, dir 1, dir 0.  N = 16 (the smallest packed N), 17 (odd: the last pair is one particle), 100;
N = 8 runs the wave-per-row kernel (one particle per lane: rng_normals<3>) through both ways into the library."""
import numpy as np
import pytest

import conv_ref as CR
import sweep_shapes as S
from sweep_shapes import CF, NEWTON

pytestmark = pytest.mark.gpu
ROWS = np.array([[0, 0, 1, 0], [1, 1, 2, 1], [2, CR.DIR_PRIOR, 0, 3], [2, 0, 3, 2], [1, 1, 0, 1], [0, 0, 2, 3]], dtype=np.int32)


@pytest.fixture(scope="module")
def env():
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    return torch, _lib, _lib.load(), R.Context(0)


def table(N):
    rng = np.random.default_rng(2100 + N)
    F, V = 3, 4
    mu = rng.uniform(-5, 5, (F, 3)) * [1, 1, 0.1]
    L = CR._chol_rows(rng, F, 3, [0.3, 0.3, 0.1]).astype(np.float32).astype(np.float64)
    mu[1, 2] = 0.0
    L[1, 3:] = 0.0                                                            # factor 1 (the dir-1 rows): no heading noise
    bel = rng.uniform(-40, 40, (V, 3, 1)) + rng.standard_normal((V, 3, N))
    bel[:, 2] = 0.0
    return {"kind": CR.P2P2, "N": N, "n_conv": len(ROWS), "seed": CR.SEED + 7 * N, "stream_offset": (1 << 32) + 40 + N, "edge_rows": (),
            "mu": np.ascontiguousarray(mu), "L": L, "bel_fixed": bel, "rows4": ROWS.copy()}


def expected(t):
    xi = CR.normals(t["seed"], t["stream_offset"], t["n_conv"], t["N"], 3)
    return CR.root_coords(CR.P2P2, CR.np_root(t, xi))


@pytest.mark.parametrize("N", (16, 17, 100))
def test_packed_sweep_returns_the_bits_of_the_reference_root(env, N):
    t = table(N)
    assert CR.launch_shape(N, len(ROWS))["packed"]
    d = S.Dev(env[0], t)
    want = expected(t)
    for solver in (NEWTON, CF):
        out = S.launch(env, d, len(ROWS), solver, "packed")[0]
        assert np.array_equal(out, want), (solver, np.argwhere(out != want)[:6].tolist())


def test_wave_per_row_kernel_returns_the_bits_of_the_reference_root(env):
    t = table(8)
    assert not CR.launch_shape(8, len(ROWS))["packed"]
    d = S.Dev(env[0], t)
    want = expected(t)
    for how in ("packed", "wave"):
        out = S.launch(env, d, len(ROWS), NEWTON, how)[0]
        assert np.array_equal(out, want), (how, np.argwhere(out != want)[:6].tolist())
