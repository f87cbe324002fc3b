"""The hypothesis rows of k_conv -- the feature-complete instantiation conv_wave_body<..., LEAN = false>: rows with a `multihypo`
alternative, a `nullhypo` probability, caller-supplied noise or a status array -- against the references of tests/hypo_ref.py, through
rome_conv_pose2pose2_dev, rome_conv_pose2point2br_dev and rome_conv_pose3pose3_dev, at every launch shape.

Shapes.  N = 1, 2, 63, 64, 65, 128, 129, 256, 257, 512: both sides of every threshold of launch_ppl_v (PPL = 1 / 2 / 4 / 8), the odd sizes
with idle lanes, N = 1 (no spread).  Row counts 1, 3, 4, 5, 11 of an 11-row table (four waves per block: surplus waves 3, 1, 0, 3, 1 redo
the last row).  Row kinds, bounds, the selection contract: hypo_ref's docstring.  EVERY particle is compared: the selection draw is exact
in double, so a kernel that took another Philox word, tag or particle index moves whole particles by metres, and each of them fails.

Every output buffer has a guard block before and after the table, pre-filled with NaN (status: -7) and checked after each launch
(tests/sweep_shapes.py); the inputs are read back after the launches and must be unchanged."""
import math

import numpy as np
import pytest

import conv_ref as CR
import hypo_ref as HR
import lin_ref
import sweep_shapes as S
from sweep_shapes import CF, GN, NEWTON

pytestmark = pytest.mark.gpu
COLUMNS = {CR.P2P2: ("alt_var", "hypo_w", "nullhypo"), CR.BR0: ("alt_var", "hypo_w", "nullhypo"), CR.P3P3: ("nullhypo",)}
SOLVERS = ((CF, False), (NEWTON, True), (GN, True))
TOL = 1e-12                                                # rome_opts_default's tol of NEWTON / GAUSS_NEWTON


@pytest.fixture(scope="module")
def env():
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    return torch, _lib, _lib.load(), R.Context(0)


def _inputs_untouched(d):
    t = d.t
    pairs = [(d.mu, t["mu"]), (d.L, t["L"]), (d.bel_fixed, t["bel_fixed"]), (d.rows4, t["rows4"])]
    if "bel_target" in t:
        pairs.append((d.bel_target, t["bel_target"]))
    pairs += [(d.hypo[k], t[k]) for k in d.hypo]
    for dev, host in pairs:
        host = np.ascontiguousarray(host).reshape(-1)
        assert np.array_equal(dev[:host.size].cpu().numpy(), host), "an input array was written"


def _mp_stride(N):
    return max(1, N // 64)


@pytest.mark.parametrize("N", HR.HYPO_N)
@pytest.mark.parametrize("kind", CR.KINDS)
def test_every_table_row_count_and_solver(env, kind, N):
    ref = HR.reference(kind, N)
    d = S.Dev(env[0], ref.table)
    assert (ref.base.scale_t <= 100.0).all()                                    # the functor check of NEWTON is asserted (tests/test_gpu_packed_sweep.py)
    for solver, status in SOLVERS:
        gn_tol = TOL if solver == GN else 0.0
        full = None
        for n in sorted(HR.ROW_COUNTS, reverse=True):
            out, st, _ = S.launch(env, d, n, solver, status=status, hypo=COLUMNS[kind])
            fig, bad = ref.check(out, gn_tol=gn_tol)
            print("HYPOROWS %s N=%d solver=%d rows=%d t %.3f r %.3f of the bound, %d entropy particles" % (kind, N, solver, n, fig["t"], fig["r"], fig["entropy"]))
            assert not bad, (solver, n, bad)
            if status:
                assert np.array_equal(st, ref.expected_status(n)), (solver, n, np.argwhere(st != 0)[:4].tolist())
            if full is None:
                full = out
                if solver == CF:                                                # against mp: every entropy particle and the mp rows of the roots
                    figm, badm = _check_mp(ref, out, _mp_stride(N))
                    assert not badm, (n, figm, badm)
            else:                                                                   # the first rows of the longer launch: the same streams, the same bits
                assert np.array_equal(out, full[:n]), (solver, n)
    if kind == CR.P2P2:                                                         # NEWTON without a status array is the closed form
        a = S.launch(env, d, HR.N_ROWS, NEWTON, hypo=COLUMNS[kind])[0]
        b = S.launch(env, d, HR.N_ROWS, CF, hypo=COLUMNS[kind])[0]
        assert np.array_equal(a, b)
    _inputs_untouched(d)


def _check_mp(ref, out, stride):
    """every stride-th particle against mpmath at hypo_ref's bounds (entropy particles: their mp value; roots: the mp rows)"""
    import mpmath as mpm
    bt, br = ref.bounds(0.0, out.shape[0])
    wt = wr = 0.0
    with mpm.workdps(lin_ref.DPS):
        for c in range(out.shape[0]):
            for i in range(0, ref.table["N"], stride):
                el = ref.mp_ent[(c, i)] if ref.entropy[c, i] else ref.base.mp[c][i] if c in ref.base.mp else None
                if el is None:
                    continue
                mt, mr = CR.distance(ref.kind, out[c, :, i], el, mp=True)
                wt = max(wt, float(mt) / bt[c, i]); wr = max(wr, float(mr) / br[c, i])
    return (wt, wr), ([] if wt <= 1.0 and wr <= 1.0 else [("against mp", wt, wr)])


@pytest.mark.parametrize("N", HR.HYPO_N)
def test_every_stored_pose2_heading_is_canonical(env, N):
    """every row kind of the Pose2Pose2 table, every solver: the stored heading lies in (-π, π] -- entropy particles of the multihypo draw
    (spreadNH x 9-26 m: ±13 rad and more before the wrap), null particles, start points stored beyond ±π, and the solved ones"""
    ref = HR.reference(CR.P2P2, N)
    d = S.Dev(env[0], ref.table)
    for solver, status in SOLVERS:
        out = S.launch(env, d, HR.N_ROWS, solver, status=status, hypo=COLUMNS[CR.P2P2])[0]
        th = out[:, 2]
        bad = np.argwhere(~((th > -math.pi) & (th <= math.pi)))
        assert len(bad) == 0, (solver, "rows", sorted(set(bad[:, 0].tolist())), [HR.KIND_OF_ROW[c] for c in sorted(set(bad[:, 0].tolist()))],
                               float(np.abs(th).max()))


@pytest.mark.parametrize("N", HR.HYPO_N)
@pytest.mark.parametrize("kind", CR.KINDS)
def test_noise_variants(env, kind, N):
    """the caller's normals (ro.rng_normals for every row and particle) give the bits of the in-kernel draw; the caller's measurement
    samples (opts.presampled) meet the reference at its bounds (the host forms z = μ + Lξ in another rounding)"""
    ref = HR.reference(kind, N)
    d = S.Dev(env[0], ref.table)
    xi = np.ascontiguousarray(np.swapaxes(ref.xi, 1, 2))                       # (C, dz, N)
    z = np.ascontiguousarray(np.swapaxes(CR.measurements(ref.effective, ref.xi), 1, 2))
    for solver, status in ((CF, False), (NEWTON, True)):
        for n in (HR.N_ROWS, 5):
            own = S.launch(env, d, n, solver, status=status, hypo=COLUMNS[kind])
            given = S.launch(env, d, n, solver, status=status, hypo=COLUMNS[kind], noise=xi[:n])
            assert np.array_equal(own[0], given[0]), (solver, n, np.argwhere(own[0] != given[0])[:4].tolist())
            assert not status or np.array_equal(own[1], given[1])
            meas = S.launch(env, d, n, solver, status=status, hypo=COLUMNS[kind], noise=z[:n], presampled=1)
            fig, bad = ref.check(meas[0])
            assert not bad, (solver, n, bad)
            assert not status or np.array_equal(meas[1], ref.expected_status(n))
    _inputs_untouched(d)


@pytest.mark.parametrize("N", (2, 64, 65, 129, 512))
@pytest.mark.parametrize("kind", CR.KINDS)
def test_columns_without_a_hypothesis_give_the_bits_of_the_plain_table(env, kind, N):
    """alt_var = -1 and nullhypo = 0 on every row, the columns present (the feature-complete instantiation, through both ways into the
    library) against the same table without the columns (the plain launch: lean k_conv at N = 2, the packed sweep from N = 16)"""
    t = HR.plain_table(HR.hypo_table(kind, N))
    assert CR.launch_shape(N, 1)["packed"] == (N >= 16)
    d = S.Dev(env[0], t)
    for solver, status in SOLVERS:
        for n in (HR.N_ROWS, 5):
            plain = S.launch(env, d, n, solver, status=status)
            for how in ("packed", "wave"):
                cols = S.launch(env, d, n, solver, how, status=status, hypo=COLUMNS[kind])
                assert np.array_equal(plain[0], cols[0]), (solver, n, how)
                assert not status or np.array_equal(plain[1], cols[1]), (solver, n, how)
    _inputs_untouched(d)


@pytest.mark.parametrize("kind", CR.KINDS)
def test_hypothesis_columns_are_refused_above_512(env, kind):
    """N = 513 leaves the register-resident kernels: with an alt_var or nullhypo column the entry point returns an error and stores nothing"""
    big = HR.hypo_table(kind, 512)
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, a[:, :, :1]], 2))
    t = dict(big, N=513, bel_fixed=pad(big["bel_fixed"]))
    if kind == CR.BR0:
        t["bel_target"] = pad(big["bel_target"])
    d = S.Dev(env[0], t)
    tries = [("nullhypo",)] if kind == CR.P3P3 else [("alt_var", "hypo_w"), ("nullhypo",), ("alt_var", "hypo_w", "nullhypo")]
    for cols in tries:
        for solver, status in ((CF, False), (NEWTON, True)):
            rc = S.launch(env, d, HR.N_ROWS, solver, status=status, hypo=cols, refused=True)
            assert rc < 0, (cols, solver, rc)
    out = S.launch(env, d, HR.N_ROWS, CF)[0]                                    # without the columns the same table runs (k_conv_big)
    assert np.isfinite(out).all()
    _inputs_untouched(d)


@pytest.mark.parametrize("N", HR.BR1_N)
def test_bearing_range_towards_the_pose_lands_on_the_ring_its_draw_names(env, N):
    """A ring of roots and inflation cycles: no unique reference root.  For every particle the mp residual of the STORED pose against the
    landmark the reference's selection names (own or alternative) is within the functor tolerance its status reports; against the other
    landmark it exceeds 6 σ (the two rings of a row never intersect: tests/test_hypo_ref_host.py)."""
    t = HR.br1_table(N)
    primary, own, other, z = HR.br1_landmarks(t)
    d = S.Dev(env[0], t)
    out, st, _ = S.launch(env, d, t["n_conv"], NEWTON, status=True, hypo=("alt_var", "hypo_w"), dir_all=1)
    assert HR.headings_in_range(out[:, 2])
    sg = t["L"][t["rows4"][:, 0]]
    has = t["alt_var"] >= 0
    # the functor is evaluated in double at coordinates up to ~20: its own rounding is a few ulp(20) on the range, ulp(π) on the bearing
    slack = 64.0 * CR.EPS * 32.0
    worst = 0.0
    for c in range(t["n_conv"]):
        for i in range(N):
            r = HR.br1_residual_mp(z[c, i], out[c, :, i], own[c, :, i])
            m = max(abs(r[0]), abs(r[1]))
            worst = max(worst, m)
            if st[c, i] == 0:
                assert m <= TOL + slack, ("status 0 but the residual exceeds tol", c, i, r)
            else:
                assert m > TOL - slack, ("status 1 but the residual is within tol", c, i, r)
            if has[c]:
                ro_ = HR.br1_residual_mp(z[c, i], out[c, :, i], other[c, :, i])
                assert max(abs(ro_[0]) / sg[c, 0], abs(ro_[1]) / sg[c, 1]) > 6.0, ("on the ring of the other landmark", c, i, ro_)
    print("HYPOROWS br->pose N=%d worst residual %.3e, status 1 on %d of %d" % (N, worst, int(st.sum()), st.size))
    assert st.mean() < 0.01, "NEWTON steps exactly onto the ring member its start selects"
    _inputs_untouched(d)
