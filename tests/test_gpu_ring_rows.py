"""The MULTI-ROOT rows of the wave-per-row kernels -- bearing-range -> pose, Point2Point2Range, Pose2Point2Range and Pose2Point2Bearing in
both directions -- against the chain references of tests/ring_ref.py (float64 on every particle, mpmath on the mp rows), through
rome_conv_pose2point2br_dev (dir_all = 1), rome_conv_point2point2range_dev, rome_conv_pose2point2range_dev and
rome_conv_pose2point2bearing_dev, under CLOSED_FORM, NEWTON and GAUSS_NEWTON.

Shapes.  N = 1, 2, 63, 64, 65, 128, 129, 256, 257, 512 (both sides of every particles-per-lane threshold of k_conv), 513 and 640
(k_conv_big with a one-particle last chunk and with whole chunks).  Row counts 1, 3, 4, 5, 11 and 37 (ten blocks: the remainder path of
xcd_contiguous_block).  `rows4` launches take the lean instantiation, column arrays the feature-complete one.  The bounds, the conditions
they rest on and the GAUSS_NEWTON slack: ring_ref's docstring; tests/test_ring_ref_host.py shows on the CPU that the bound rejects a
wrong summation, a world-frame entropy, a heading left out of the spread, a jitter stream from the factor index and a dropped cycle.

Every output buffer has a guard block before and after the table, pre-filled with NaN (status: -7) and checked after each launch
(tests/sweep_shapes.py); the inputs are read back after the launches and must be unchanged."""
import numpy as np
import pytest

import hypo_ref as HR
import ring_ref as RR
import sweep_shapes as S
from sweep_shapes import CF, GN, NEWTON

pytestmark = pytest.mark.gpu
SOLVERS = ((CF, False), (NEWTON, True), (GN, True))
TOL = RR.TOL                                               # rome_opts_default's tol of NEWTON / GAUSS_NEWTON
HOWS = ("packed", "wave")                                  # rows4: the lean instantiation; column arrays: the feature-complete one


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


def _opts(t, **kw):
    o = {"inflate_cycles": t["cycles"], "inflation": t["inflation"]}
    o.update(kw)
    return o


def _gn(solver):
    return TOL if solver == GN else 0.0


def _line(kind, N, what, fig):
    print("RINGROWS %s N=%d %s worst/bound t %.3f r %.3f%s" % (kind, N, what, fig["t"], fig["r"],
                                                               " mp %.3f %.3f" % (fig["mp_t"], fig["mp_r"]) if "mp_t" in fig else ""))


# ------------------------------------------------------------------------------------------------------------ 1. every shape
@pytest.mark.parametrize("N", RR.RING_N)
@pytest.mark.parametrize("kind", RR.KINDS)
def test_every_shape_solver_and_instantiation(env, kind, N):
    ref = RR.reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    for solver, status in SOLVERS:
        outs = {}
        for how in HOWS:
            out, st, _ = S.launch(env, d, t["n_conv"], solver, how, status=status, **_opts(t))
            fig, bad = ref.check(out, gn_tol=_gn(solver), mp=ref.mp)
            _line(kind, N, "solver=%d %s" % (solver, how), fig)
            assert not bad, (solver, how, bad)
            if status:                                                          # condition (d): every solved particle reports 0
                assert not st.any(), (solver, how, np.argwhere(st != 0)[:4].tolist())
            outs[how] = (out, st)
        assert np.array_equal(outs["packed"][0], outs["wave"][0]), (solver, "lean and feature-complete differ")
        assert not status or np.array_equal(outs["packed"][1], outs["wave"][1])
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 2. row counts
@pytest.mark.parametrize("N", RR.RING_N)
@pytest.mark.parametrize("kind", RR.KINDS)
def test_row_counts_and_windows(env, kind, N):
    """the rows of a short launch equal the same rows of the long one bit for bit (the streams are stream_offset + row), from row 0 and
    in windows that start later; the long one is held to the reference"""
    ref = RR.reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    for solver, status in ((CF, False), (GN, True)):
        full, fst, _ = S.launch(env, d, t["n_conv"], solver, status=status, **_opts(t))
        assert not ref.check(full, gn_tol=_gn(solver))[1]
        for how in HOWS:
            for row0, n in [(0, n) for n in HR.ROW_COUNTS[:-1]] + [(3, 5), (7, 4), (10, 1)]:
                out, st, _ = S.launch(env, d, n, solver, how, status=status, row0=row0, **_opts(t))
                assert np.array_equal(out, full[row0:row0 + n]), (solver, how, row0, n)
                assert not status or np.array_equal(st, fst[row0:row0 + n])
    _inputs_untouched(d)


@pytest.mark.parametrize("N", RR.LONG_N)
@pytest.mark.parametrize("kind", RR.KINDS)
def test_ten_blocks(env, kind, N):
    """37 rows: ten blocks, more than eight and no multiple of eight -- the remainder path of the per-block XCD remapping"""
    ref = RR.reference(kind, N, RR.N_LONG)
    t = ref.table
    d = S.Dev(env[0], t)
    for solver, status in SOLVERS:
        for how in HOWS:
            out, st, _ = S.launch(env, d, RR.N_LONG, solver, how, status=status, **_opts(t))
            fig, bad = ref.check(out, gn_tol=_gn(solver), mp=ref.mp if solver == CF else None)
            _line(kind, N, "37 rows solver=%d %s" % (solver, how), fig)
            assert not bad, (solver, how, bad)
            assert not status or not st.any()
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 3. cycles
@pytest.mark.parametrize("N", (64, 65, 257, 513))
@pytest.mark.parametrize("kind", RR.KINDS)
def test_cycles_and_inflation(env, kind, N):
    ref = RR.reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    for solver, status in SOLVERS:
        got = {}
        for cyc, infl in ((1, 0.0), (3, 0.0), (2, t["inflation"]), (3, t["inflation"])):
            v = ref.variant(cyc, infl)
            out, st, _ = S.launch(env, d, t["n_conv"], solver, status=status, inflate_cycles=cyc, inflation=infl)
            fig, bad = ref.check(out, gn_tol=_gn(solver), ref=v["out"], mp=v["mp"])
            _line(kind, N, "cycles=%d inflation=%g solver=%d" % (cyc, infl, solver), fig)
            assert not bad, (solver, cyc, infl, bad)
            assert not status or not st.any()
            got[(cyc, infl)] = out
        # the projection is idempotent: three cycles without inflation are one, within the bound
        one = np.ascontiguousarray(np.swapaxes(got[(1, 0.0)], 1, 2))
        assert not ref.check(got[(3, 0.0)], gn_tol=_gn(solver), ref=one)[1], solver
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 4. noise sources
@pytest.mark.parametrize("N", RR.RING_N)
@pytest.mark.parametrize("kind", RR.KINDS)
def test_noise_sources(env, kind, N):
    """the reference's normals handed in (`noise`), and its measurements (`presampled`): the same chain, the same bound"""
    ref = RR.reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    xi = np.ascontiguousarray(np.swapaxes(ref.xi, 1, 2))
    z = np.ascontiguousarray(np.swapaxes(ref.z, 1, 2))
    for solver, status in SOLVERS:
        for how in HOWS:
            for what, kw in (("normals", {"noise": xi}), ("measurements", {"noise": z, "presampled": 1})):
                out, st, _ = S.launch(env, d, t["n_conv"], solver, how, status=status, **_opts(t, **kw))
                fig, bad = ref.check(out, gn_tol=_gn(solver))
                assert not bad, (solver, how, what, bad)
                assert not status or not st.any()
    _line(kind, N, "noise handed in", fig)
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("kind", RR.KINDS)
def test_edges(env, kind):
    """edge_table(kind): presampled measurements, one cycle, no inflation -- every particle an independent case; the output where the
    contract says, the status inside the window the mp residual of the stored point allows, ρ <= 0 of a range row: 1 under NEWTON and
    GAUSS_NEWTON, 0 under CLOSED_FORM"""
    ref = RR.edge_reference(kind)
    t = ref.table
    d = S.Dev(env[0], t)
    z = np.ascontiguousarray(np.swapaxes(ref.z, 1, 2))
    for solver in (CF, NEWTON, GN):
        for how in HOWS:
            out, st, _ = S.launch(env, d, t["n_conv"], solver, how, status=True, noise=z, presampled=1, inflate_cycles=1, inflation=0.0)
            fig, bad = ref.check(out, gn_tol=_gn(solver), mp=ref.mp)
            _line(kind, RR.EDGE_N, "edges solver=%d %s" % (solver, how), fig)
            assert not bad, (solver, how, bad, [(ref.z[c, i].tolist(), ref.fx[c, i].tolist(), ref.start[c, i].tolist(), out[c, :, i].tolist(),
                                                 ref.ref[c, i].tolist()) for c, i in (bad[0][1] if bad[0][0] == "value" else [])])
            if solver == CF:
                assert not st.any()
                continue
            must0, must1 = ref.status_window(out, TOL)
            wrong = (must0 & (st != 0)) | (must1 & (st != 1))
            assert not wrong.any(), (solver, how, [(int(c), int(i), int(st[c, i]), ref.z[c, i].tolist(), ref.fx[c, i].tolist(),
                                                    ref.start[c, i].tolist()) for c, i in np.argwhere(wrong)[:4]])
            if RR.STEP[kind] == "range":
                assert must1[~(ref.z[..., 0] > 0.0)].all() and (~(ref.z[..., 0] > 0.0)).any()
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 6. degenerate belief
@pytest.mark.parametrize("N", (2, 65, 513))
@pytest.mark.parametrize("kind", RR.KINDS)
def test_identical_start_particles(env, kind, N):
    """N copies of one particle: sd = 0 on both sides, the spread is exactly inflation · 1"""
    ref = RR.identical_reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    one = ref.variant(1, t["inflation"])
    for solver, status in SOLVERS:
        for how in HOWS:
            out, st, _ = S.launch(env, d, t["n_conv"], solver, how, status=status, inflate_cycles=1, inflation=t["inflation"])
            fig, bad = ref.check(out, gn_tol=_gn(solver), ref=one["out"], mp=one["mp"])
            assert not bad, (solver, how, "one cycle", bad)
            out, st, _ = S.launch(env, d, t["n_conv"], solver, how, status=status, **_opts(t))
            fig, bad = ref.check(out, gn_tol=_gn(solver), mp=ref.mp)
            assert not bad, (solver, how, bad)
            assert not status or not st.any()
    _line(kind, N, "identical start particles", fig)
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 7. nullhypo
@pytest.mark.parametrize("N", (2, 64, 65, 129, 257, 512))
@pytest.mark.parametrize("kind", RR.KINDS)
def test_nullhypo_column(env, kind, N):
    """the selection is exact (a wrong draw moves whole particles by metres); null particles skip the cycles, stay in the statistic,
    carry status 0 and hypo_ref's entropy bound; solved particles are held to the chain bound"""
    ref = RR.reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    v = ref.variant(nullhypo=True)
    assert v["null"].any() and not v["null"].all()
    for solver, status in SOLVERS:
        for how in HOWS:
            out, st, _ = S.launch(env, d, t["n_conv"], solver, how, status=status, hypo=("nullhypo",), **_opts(t))
            fig, bad = ref.check(out, gn_tol=_gn(solver), ref=v["out"], mp=v["mp"], add=v["add"])
            assert not bad, (solver, how, bad)
            assert not status or not st.any()
    _line(kind, N, "nullhypo, %d null particles" % int(v["null"].sum()), fig)
    _inputs_untouched(d)


@pytest.mark.parametrize("kind", RR.KINDS)
def test_nullhypo_and_mirrors_are_refused_above_512(env, kind):
    t = RR.reference(kind, 513).table
    d = S.Dev(env[0], t)
    n = t["n_conv"]
    for solver, status in ((CF, False), (NEWTON, True), (GN, True)):
        for how in HOWS:
            assert S.launch(env, d, n, solver, how, status=status, hypo=("nullhypo",), refused=True, **_opts(t)) != 0
            assert S.launch(env, d, n, solver, how, status=status, mirror=("map", [k % 3 - 1 for k in range(n)]), refused=True, **_opts(t)) != 0
            assert S.launch(env, d, n, solver, how, status=status, mirror=("rows", [9, 2]), refused=True, **_opts(t)) != 0
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 8. mirrors
@pytest.mark.parametrize("N", (64, 65, 512))
@pytest.mark.parametrize("kind", RR.KINDS)
def test_mirror_blocks(env, kind, N):
    ref = RR.reference(kind, N)
    t = ref.table
    d = S.Dev(env[0], t)
    n = t["n_conv"]
    slots = [-1, 3, -1, 0, -1, -1, 4, 1, -1, -1, 2]
    for solver, status in SOLVERS:
        plain = S.launch(env, d, n, solver, status=status, **_opts(t))[0]
        for how in HOWS:
            out, _, mb = S.launch(env, d, n, solver, how, status=status, mirror=("map", slots), **_opts(t))
            assert np.array_equal(out, plain)
            for c, m in enumerate(slots):
                assert m < 0 or np.array_equal(mb[m], out[c]), (solver, how, c, m)
            listed = [10, 0, 5, 7]
            out, _, mb = S.launch(env, d, n, solver, how, status=status, mirror=("rows", listed), **_opts(t))
            assert np.array_equal(out, plain)
            assert all(np.array_equal(mb[k], out[c]) for k, c in enumerate(listed)), (solver, how)
    _inputs_untouched(d)


# ------------------------------------------------------------------------------------------------------------ 9. alignment
@pytest.mark.parametrize("N", (65, 129))
@pytest.mark.parametrize("kind", RR.KINDS)
def test_alignment(env, kind, N):
    """`out` and the beliefs one double off their 16-byte alignment: the same bits"""
    ref = RR.reference(kind, N)
    t = ref.table
    d, ds = S.Dev(env[0], t), S.Dev(env[0], t, shift=True)
    for solver, status in SOLVERS:
        for how in HOWS:
            a = S.launch(env, d, t["n_conv"], solver, how, status=status, **_opts(t))
            b = S.launch(env, ds, t["n_conv"], solver, how, status=status, shift=True, **_opts(t))
            assert np.array_equal(a[0], b[0]), (solver, how)
            assert not status or np.array_equal(a[1], b[1])
    _inputs_untouched(d)
