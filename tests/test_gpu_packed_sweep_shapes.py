"""The packed sweep k_conv_flat against the wave-per-row kernel k_conv, bit for bit, at the smallest shapes at which its addressing or its
constant staging can go wrong, and against the root references of tests/conv_ref.py at that file's bounds.  Launch helpers, the two
ways into the library and the case list: tests/sweep_shapes.py.

Shapes.  N = 16 (H = 8 < NK: two staging passes for Pose2, four for Pose3), 18 (H = 9 = NK of Pose2: the second pass is skipped, Pose3
still takes three), 100 (CPB = 5), 101 (odd: no 16-byte accesses, the last pair is one particle), 512 (H = 256: one row per block);
rows = 1, CPB - 1, CPB, CPB + 1, 8 CPB + 3.  The tables are conv_ref's shape tables: dir 0 / dir 1 / prior rows interleaved, the last block
of the store among the fixed variables, factor and variable indices out of row order.

Range factors have a ring of roots and never take the packed kernel; for them the plain (`rows4`) and the feature-complete instantiation
of k_conv are compared, which share the measurement draw with the packed sweep (box_muller).

Beyond 4 GiB: a belief store and a proposal array whose byte offsets pass 2^32 (skipped below 12 GiB of free device memory).

tests/golden/packed_sweep_bits.json holds the sha256 of the proposal bytes of a dozen of these tables, written by
scripts/packed_sweep_bits.py; the proposals are bit-for-bit what they were when it was written."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import conv_ref as CR
import sweep_shapes as S
from sweep_shapes import CF, GN, NEWTON

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = {CR.P2P2: ((CF, False), (NEWTON, True), (GN, True)), CR.BR0: ((CF, False), (GN, True)), CR.P3P3: ((CF, False),)}
GIB = 1 << 30


@pytest.fixture(scope="module")
def env():
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    return torch, _lib, _lib.load(), R.Context(0)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), ("proposals differ", what)
    assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1]), ("status differs", what)


@pytest.mark.parametrize("N", S.SHAPE_N)
@pytest.mark.parametrize("kind", CR.KINDS)
def test_packed_sweep_equals_the_wave_per_row_kernel(env, kind, N):
    ref = S.reference(kind, N)
    d = S.Dev(env[0], ref.table)
    ns = S.n_conv_cases(N)
    assert ns[-1] <= ref.table["n_conv"] and CR.launch_shape(N, ns[-1])["nb"] % 8 != 0 and CR.launch_shape(N, 1)["packed"]
    fixed = ref.table["rows4"][:ns[-1], 2]
    assert (fixed == len(ref.table["bel_fixed"]) - 1).any(), "a row reads the last block of the store"
    if kind != CR.BR0:
        assert (ref.table["rows4"][:ns[-1], 1] == CR.DIR_PRIOR).any()
    for solver, status in SOLVERS[kind]:
        for n in ns:
            packed = S.launch(env, d, n, solver, "packed", status=status)
            wave = S.launch(env, d, n, solver, "wave", status=status)
            _same(packed, wave, (solver, n))
            fig, bad = ref.check(packed[0], gn_tol=1e-12 if solver == GN else 0.0)
            assert not bad, (solver, n, bad)


@pytest.mark.parametrize("N", (18, 100, 101))
@pytest.mark.parametrize("kind", (CR.P2P2, CR.BR0))
def test_mirror_blocks_and_unaligned_views(env, kind, N):
    ref = S.reference(kind, N)
    cpb = CR.launch_shape(N, 1)["CPB"]
    n = 8 * cpb + 3
    a, b = S.Dev(env[0], ref.table), S.Dev(env[0], ref.table, shift=True)
    slots = np.full(n, -1, dtype=np.int32)
    rows = [0, cpb - 1, cpb, 2 * cpb + 1, n - cpb - 1, n - 1]                    # first and last row, both sides of a block boundary
    for m, r in zip((5, 0, 3, 6, 1, 2), rows):                                   # slot 4 stays unused
        slots[r] = m
    four = [n - 1, cpb, 0, cpb - 1]
    for solver in (CF, GN):
        plain = S.launch(env, a, n, solver)
        for how in ("packed", "wave"):
            for dev, shift in ((a, False), (b, True)):                           # shift: store, out and mirror_out at an odd element offset
                out, _, mir = S.launch(env, dev, n, solver, how, shift=shift, mirror=("map", slots))
                assert np.array_equal(out, plain[0]), (solver, how, shift)
                for r in rows:
                    assert np.array_equal(mir[slots[r]], out[r]), (solver, how, shift, r)
                assert np.isnan(mir[4]).all()
                out, _, mir = S.launch(env, dev, n, solver, how, shift=shift, mirror=("rows", four))
                assert np.array_equal(out, plain[0]), (solver, how, shift)
                for m, r in enumerate(four):
                    assert np.array_equal(mir[m], out[r]), (solver, how, shift, r)


@pytest.mark.parametrize("N", (16, 100, 512))
def test_unaligned_views_with_status(env, N):
    ref = S.reference(CR.P2P2, N)
    n = S.n_conv_cases(N)[-1]
    a, b = S.Dev(env[0], ref.table), S.Dev(env[0], ref.table, shift=True)
    for solver in (NEWTON, GN):
        want = S.launch(env, a, n, solver, status=True)
        _same(want, S.launch(env, b, n, solver, status=True, shift=True), (solver, "packed"))
        _same(want, S.launch(env, b, n, solver, "wave", status=True, shift=True), (solver, "wave"))


@pytest.mark.parametrize("N", (16, 100, 101))
def test_range_rows_plain_and_feature_complete_kernel_agree(env, N):
    """Point2Point2Range, both directions: the `rows4` launch (plain k_conv) against the column arrays (feature-complete k_conv)"""
    torch, _lib, lib, ctx = env
    rng = np.random.default_rng(700 + N)
    F, V, n = 5, 7, 23
    c = np.arange(n)
    rows = np.stack([(3 * c + 1) % F, c % 2, (5 * c + 6) % V, (2 * c + 3) % V], 1).astype(np.int32)
    assert (rows[:, 2] == V - 1).any()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mu, sg = up(rng.uniform(5.0, 15.0, F)), up(rng.uniform(0.1, 0.5, F))
    bel = up(rng.uniform(-20, 20, (V, 2, 1)) + rng.standard_normal((V, 2, N)))
    r4, cols = up(rows), [up(rows[:, k]) for k in range(4)]
    got = []
    for how in ("rows4", "columns"):
        o = _lib.default_opts(CF, n_particles=N, seed=CR.SEED + N, stream_offset=(1 << 33) + 5)
        out = torch.full(((n + 2) * 2 * N,), float("nan"), dtype=torch.float64, device="cuda")
        T = _lib.ConvDev()
        T.n_conv = n
        T.mu, T.L, T.bel_fixed, T.bel_target = mu.data_ptr(), sg.data_ptr(), bel.data_ptr(), bel.data_ptr()
        T.out = out.data_ptr() + 8 * 2 * N
        if how == "rows4":
            T.rows4 = r4.data_ptr()
        else:
            T.factor, T.dir, T.fixed_var, T.target_var = [k.data_ptr() for k in cols]
        torch.cuda.synchronize()
        _lib.check(lib.rome_conv_point2point2range_dev(ctx.handle, C.byref(o), C.byref(T)), ctx.handle)
        ctx.synchronize()
        h = out.cpu().numpy()
        assert np.isnan(h[:2 * N]).all() and np.isnan(h[(n + 1) * 2 * N:]).all() and np.isfinite(h[2 * N:(n + 1) * 2 * N]).all()
        got.append(h[2 * N:(n + 1) * 2 * N])
    assert np.array_equal(got[0], got[1])


# --------------------------------------------------------------------------------------------------------------- beyond 4 GiB
def _need(torch, gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip("needs %d GiB of free device memory, %.1f free" % (gib, free / GIB))


def test_belief_store_beyond_4_gib(env):
    """ten rows whose fixed and target variables are the last two blocks of a Pose2 store of ceil(2^32 / (3 N 8)) + 2 blocks (allocated, not
    filled): the same bits as from a two-block store"""
    torch, _lib, lib, ctx = env
    _need(torch, 12)
    N = 100
    t = dict(S.reference(CR.P2P2, N).table)
    nblk = -(-(1 << 32) // (3 * N * 8)) + 2
    assert (nblk - 2) * 3 * N * 8 >= 1 << 32
    rows = t["rows4"][:10].copy()
    rows[:, 2] = np.arange(10) % 2
    rows[:, 3] = (np.arange(10) // 2) % 2
    t["rows4"], t["n_conv"], t["bel_fixed"] = rows, 10, t["bel_fixed"][3:5].copy()
    small = S.Dev(torch, t)
    store = torch.empty(nblk * 3 * N, dtype=torch.float64, device="cuda")
    store[(nblk - 2) * 3 * N:] = torch.from_numpy(t["bel_fixed"].reshape(-1)).cuda()
    big = S.Dev(torch, t)
    shifted = rows.copy()
    shifted[:, 2:] += nblk - 2
    big.rows4 = torch.from_numpy(shifted).cuda()
    big.cols = [torch.from_numpy(np.ascontiguousarray(shifted[:, k])).cuda() for k in range(4)]
    big.bel_fixed = big.bel_target = store
    for solver, status in SOLVERS[CR.P2P2]:
        want = S.launch(env, small, 10, solver, status=status)
        _same(want, S.launch(env, big, 10, solver, status=status), (solver, "packed"))
        _same(want, S.launch(env, big, 10, solver, "wave", status=status), (solver, "wave"))
    del store


def test_proposals_beyond_4_gib(env):
    """a table of ceil(2^32 / (3 N 8)) + 8 rows at N = 100: its last 16 rows are the bits of the same rows run as a short table"""
    torch, _lib, lib, ctx = env
    _need(torch, 12)
    N = 100
    t = dict(S.reference(CR.P2P2, N).table)
    base = t["rows4"]
    nrow = -(-(1 << 32) // (3 * N * 8)) + 8
    assert (nrow - 16) * 3 * N * 8 < 1 << 32 < (nrow - 1) * 3 * N * 8             # the 16 rows straddle the 4 GiB line
    rows = np.ascontiguousarray(base[np.arange(nrow) % len(base)])
    d = S.Dev(torch, t)
    r4 = torch.from_numpy(rows).cuda()
    out = torch.empty(nrow * 3 * N, dtype=torch.float64, device="cuda")
    out[(nrow - 17) * 3 * N:] = float("nan")
    o = _lib.default_opts(CF, n_particles=N, seed=t["seed"], stream_offset=t["stream_offset"])
    T = _lib.ConvDev()
    T.n_conv = nrow
    T.mu, T.L, T.bel_fixed, T.bel_target = d.mu.data_ptr(), d.L.data_ptr(), d.bel_fixed.data_ptr(), d.bel_target.data_ptr()
    T.rows4, T.out = r4.data_ptr(), out.data_ptr()
    torch.cuda.synchronize()
    _lib.check(lib.rome_conv_pose2pose2_dev(ctx.handle, C.byref(o), C.byref(T)), ctx.handle)
    ctx.synchronize()
    tail = out[(nrow - 16) * 3 * N:].cpu().numpy().reshape(16, 3, N)
    head = out[:16 * 3 * N].cpu().numpy().reshape(16, 3, N)
    del out
    t2 = dict(t)
    t2["rows4"], t2["n_conv"], t2["stream_offset"] = rows[nrow - 16:], 16, t["stream_offset"] + nrow - 16
    short = S.launch(env, S.Dev(torch, t2), 16, CF)[0]
    assert np.array_equal(tail, short)
    assert np.array_equal(head, S.launch(env, d, 16, CF)[0])


# --------------------------------------------------------------------------------------------------------------- recorded bits
def test_proposal_bits_are_the_recorded_ones(env):
    with open(os.path.join(ROOT, "tests", "golden", "packed_sweep_bits.json")) as f:
        want = json.load(f)["sha256"]
    got = S.golden_hashes(env)
    assert sorted(got) == sorted(want) and len(got) >= 12
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, diff
