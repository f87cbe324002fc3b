"""tests/ring_ref.py on the CPU: the float64 chains against the existing restatements (range_ref, bearing_ref, the C oracle's bearing-range
convolution towards the pose), the measured reference error under its ceiling, the conditions (a)-(f) of the module docstring on the
reference alone, the launch arithmetic of the shapes the GPU test runs, and the discrimination of the bound: every mutant of the chain
leaves it on every kind it applies to.  `-s` prints dev per table."""
import math

import numpy as np
import pytest

import bearing_ref
import conv_ref as CR
import hypo_ref as HR
import oracle as ro
import range_ref
import ring_ref as RR

EPS = RR.EPS
TIE_N = (2, 65)


def _soa(out):
    return np.ascontiguousarray(np.swapaxes(out, 1, 2))


def _blocks(t):
    rows = t["rows4"]
    return t["bel_fixed"][rows[:, 2]], t.get("bel_target", t["bel_fixed"])[rows[:, 3]]


# ------------------------------------------------------------------------------------------------------------ ties to the older restatements
@pytest.mark.parametrize("N", TIE_N)
@pytest.mark.parametrize("kind", RR.KINDS)
def test_chain_agrees_with_the_existing_restatement(kind, N):
    """range_ref.conv / bearing_ref.conv (per-row restatements over the oracle's primitives) and ro.conv_pose2point2br(direction=1) on the
    ring_table, within the kernel's bound: the new reference and the old ones cannot drift apart silently"""
    ref = RR.reference(kind, N)
    t = ref.table
    f = t["rows4"][:, 0]
    oo = ro.make_opts(N=N, solver=ro.SOLVER_CLOSED_FORM, seed=t["seed"], stream_offset=t["stream_offset"], inflate_cycles=t["cycles"],
                      inflation=t["inflation"])
    fixed, target = _blocks(t)
    if kind == "br1":
        old = ro.conv_pose2point2br(oo, 1, t["mu"], t["L"], t["bel_fixed"], t["bel_target"], t["rows4"][:, 2], t["rows4"][:, 3], factor=f)
    else:
        mod = bearing_ref if kind in ("pb0", "pb1") else range_ref
        old, st = mod.conv(oo, t["mu"][f], t["L"][f], fixed, target, 0)
        assert not st.any()
    fig, bad = ref.check(old)
    print("RINGREF tie %s N=%d t %.3f r %.3f of the bound" % (kind, N, fig["t"], fig["r"]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ dev and the conditions
@pytest.mark.parametrize("kind", RR.KINDS)
def test_dev_and_conditions_of_every_ring_table(kind):
    worst = [0.0, 0.0]
    for N in RR.RING_N:
        for n_conv in (RR.N_ROWS,) + ((RR.N_LONG,) if N in RR.LONG_N else ()):
            ref = RR.reference(kind, N, n_conv)
            t = ref.table
            dt, dr = ref.dev["t"] / EPS, ref.dev["r"] / EPS
            worst = [max(worst[0], dt), max(worst[1], dr)]
            fig = ref.mp_fig
            print("RINGREF %s N=%d rows=%d dev %.2f / %.2f eps, mp rows %s, min ‖t-a‖/need %.2f, min jittered |r| %.1e, scale %.2f / %.2f"
                  % (kind, N, n_conv, dt, dr, ref.mp_rows, fig["min_ratio"], fig["min_jit_r"], ref.scale_t.max(), ref.scale_r.max()))
            assert dt <= RR.DEV_CEILING and dr <= RR.DEV_CEILING
            assert ref.rel_bound["t"] == RR.ULP64 and ref.rel_bound["r"] == RR.ULP64        # every bound is the floor
            assert fig["min_ratio"] >= 1.0                                                  # (a)
            if kind in RR.HAS_RHO:
                assert (ref.z[..., -1] > 0.0).all()                                         # (b)
            if N > 1:
                assert ref.seq["sd"].min() >= 1e-7 and ref.pair["sd"].min() >= 1e-7         # (b)
                assert fig["min_jit_r"] >= RR.GN_MARGIN * RR.TOL                            # (f)
                assert ref.seq["max_dth"] <= math.pi - RR.WRAP_CLEAR
            assert RR.ULP64 * max(ref.scale_t.max(), ref.scale_r.max()) < RR.TOL / 8.0      # (d)
            assert fig["max_final_r"] < 1e-40                                               # (d): the reference root is a root
            # (c): check() masks nothing -- a NaN anywhere fails it
            probe = _soa(ref.ref).copy()
            probe[-1, 0, -1] = np.nan
            assert ref.check(probe)[1] and not ref.check(_soa(ref.ref))[1]
            # the table's shape: indices out of row order, the last blocks in use, one Uniform row
            rows = t["rows4"]
            assert not np.array_equal(rows[:, 0], np.arange(n_conv)) and rows[:, 2:].max() == RR.V_STORE - 1
            assert (t["L"].reshape(-1, RR.DIMS[kind][0])[rows[RR.ROW_UNIFORM, 0]] < 0).any()
    print("RINGREF %s worst dev %.2f / %.2f eps" % (kind, worst[0], worst[1]))


@pytest.mark.parametrize("kind", RR.KINDS)
def test_special_rows_are_what_they_claim(kind):
    ref = RR.reference(kind, 65)
    dz, df, dt = RR.DIMS[kind]
    if dt == 3:
        th = ref.table["bel_target"][ref.table["rows4"][RR.ROW_STRADDLE, 3], 2]
        assert (th > 3.0).any() and (th < -3.0).any() and np.abs(CR._np_remainder(th - th[0])).max() < 1.0
    if df == 3:
        th = ref.fx[RR.ROW_STRADDLE, :, 2]
        assert (th > 3.0).any() and (th < -3.0).any()
    if kind == "pb0":
        assert (ref.fx[RR.ROW_BEYOND, :, 2] + ref.z[RR.ROW_BEYOND, :, 0] > math.pi).all()
    if kind in ("br1", "pb1"):
        assert (ref.z[RR.ROW_BEYOND, :, 0] > math.pi).any()


@pytest.mark.parametrize("kind", RR.KINDS)
def test_identical_start_particles_fall_back_to_spread_one(kind):
    """(e): N copies of one particle -> sd is exactly 0 in every evaluation, the spread is inflation · 1"""
    for N in (2, 65, 513):
        ref = RR.identical_reference(kind, N)
        assert (ref.seq["sd"][:, 0] == 0.0).all() and (ref.pair["sd"][:, 0] == 0.0).all()
        assert ref.dev["t"] / EPS <= RR.DEV_CEILING and ref.dev["r"] / EPS <= RR.DEV_CEILING
        one = ref.run("seq", cycles=1)["out"]
        U = np.stack([ref.uniforms(c)[0] for c in range(ref.C)])
        moved = np.stack([RR._np_step(kind, ref.z[c], ref.fx[c], RR._np_entropy(kind, ref.start[c], ref.inflation * 1.0 * (U[c] - 0.5)))
                          for c in range(ref.C)])
        assert np.array_equal(one, moved)


@pytest.mark.parametrize("kind", RR.KINDS)
def test_edge_table_and_variants(kind):
    e = RR.edge_reference(kind)
    print("RINGREF edge %s: %d cases, dev %.2f / %.2f eps" % (kind, e.table["n_cases"], e.dev["t"] / EPS, e.dev["r"] / EPS))
    assert e.dev["t"] / EPS <= RR.DEV_CEILING and e.dev["r"] / EPS <= RR.DEV_CEILING
    assert sorted(e.mp_rows) == list(range(e.C))
    ref = RR.reference(kind, 65)
    for kw in ({"cycles": 1, "inflation": 0.0}, {"cycles": 2}, {"nullhypo": True}):
        v = ref.variant(**kw)
        fig, bad = ref.check(_soa(v["out"]), ref=v["out"], mp=v["mp"])
        assert not bad and fig["mp_t"] <= 0.125 and fig["mp_r"] <= 0.125, (kw, fig)         # the float64 variant within 8 eps of mp
    v = ref.variant(nullhypo=True)
    p = ref.table["nullhypo"]
    assert (v["null"][p == 0.0] == 0).all() and v["null"][p == 1.0].all() and 0.1 < v["null"][p == 0.3].mean() < 0.5
    # the projection is idempotent: three cycles without inflation are one
    a, b = ref.variant(cycles=1, inflation=0.0)["out"], ref.variant(cycles=3, inflation=0.0)["out"]
    assert not ref.check(_soa(b), ref=a)[1]


# ------------------------------------------------------------------------------------------------------------ launch arithmetic
def _xcd(b, nb):
    q, r = nb >> 3, nb & 7
    return (b & 7) * q + min(b & 7, r) + (b >> 3)


def test_launch_arithmetic():
    assert RR.RING_N[:-2] == HR.HYPO_N
    assert [HR.launch_ppl(N) for N in HR.HYPO_N] == [1, 1, 1, 1, 2, 2, 4, 4, 8, 8] == [HR.PPL_OF[N] for N in HR.HYPO_N]
    assert RR.big_chunks(513) == (5, 1) and RR.big_chunks(640) == (5, 128)              # k_conv_big: a one-particle last chunk, whole chunks
    assert [RR.blocks(n) for n in HR.ROW_COUNTS + (RR.N_LONG,)] == [1, 1, 1, 2, 3, 10]  # a partial / full / just-started block, three, ten
    assert RR.blocks(RR.N_LONG) > 8 and RR.blocks(RR.N_LONG) % 8 != 0                   # the remainder path of xcd_contiguous_block
    for nb in (1, 2, 3, 10):
        assert sorted(_xcd(b, nb) for b in range(nb)) == list(range(nb))
    assert [_xcd(b, 10) for b in range(10)] == [0, 2, 4, 5, 6, 7, 8, 9, 1, 3]


# ------------------------------------------------------------------------------------------------------------ discrimination
MUTANTS = {"no_heading": "pose", "heading_unwrapped": "pose", "var_over_n": "all", "world_frame": "pose", "factor_stream": "all",
           "skip_last": "all", "pb1_plus_b": ("pb1",), "br1_no_rewrap": ("br1",)}


def _applies(mutant, kind):
    to = MUTANTS[mutant]
    return to == "all" or (to == "pose" and RR.DIMS[kind][2] == 3) or kind in to


@pytest.mark.parametrize("N", RR.LONG_N)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_leaves_the_bound(mutant, N):
    for kind in RR.KINDS:
        if not _applies(mutant, kind):
            continue
        ref = RR.reference(kind, N)
        out = ref.run("seq", mutant=mutant)["out"]
        fig, bad = ref.check(_soa(out), gn_tol=RR.TOL)                                   # at the widest bound any solver is held to
        rows = sorted({r[0] for b in bad if b[0] == "value" for r in b[1]} | {r[0] for b in bad if b[0] != "value" for r in b[1]})
        print("RINGREF mutant %s %s N=%d: t %.3g r %.3g of the bound, rows %s" % (mutant, kind, N, fig["t"], fig["r"], rows))
        assert bad, (mutant, kind, N, "the bound cannot tell this mutant from the truth")
