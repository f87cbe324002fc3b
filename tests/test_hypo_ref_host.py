"""The hypothesis-row references of tests/hypo_ref.py check one another on the CPU: float64 against mpmath on every table (roots of the
effective tables, entropy particles, the statistic in two summation orders), the reference against the C oracle where the oracle can
express the table (one global nullhypo; Pose2Pose2 and bearing-range alternatives), the heading range of both, the launch arithmetic and
the content of the tables.  Run with -s, it prints the figures recorded in hypo_ref's docstring; the GPU tests take their bounds from the
same objects."""
import math
import os
import re

import numpy as np
import pytest

import conv_ref as CR
import hypo_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CEILING = 8.0 * CR.EPS
ORACLE_N = (1, 2, 64, 65, 257)


def test_launch_arithmetic_each_n_lands_in_its_ppl():
    src = open(os.path.join(ROOT, "rome.jl_amd", "csrc", "rome_conv.hpp")).read()
    got = re.findall(r"(?:if|else if) \(a\.N <= (\d+)\)\s+hipLaunchKernelGGL\(\(k_conv<FP, SOLVER, (\d+), LEAN>\)", src)
    assert [(int(a), int(b)) for a, b in got] == [(64, 1), (128, 2), (256, 4), (512, 8)]
    assert int(re.search(r"#define ROME_WPB (\d+)", src).group(1)) == HR.WPB
    assert "if (a.alt_var || a.nullhypo || a.n_mirror > 0 || a.mirror_map) return hipErrorInvalidValue;" in src
    for N in HR.HYPO_N:
        assert HR.launch_ppl(N) == HR.PPL_OF[N], N
    assert sorted(set(HR.PPL_OF.values())) == [1, 2, 4, 8]
    for ppl, edge in ((1, 64), (2, 128), (4, 256), (8, 512)):                    # both sides of every threshold
        assert HR.PPL_OF[edge] == ppl and (edge == 512 or HR.PPL_OF[edge + 1] == 2 * ppl)
    # row counts: one wave, a partial, a full and a just-started last block (surplus waves 3, 1, 0, 3, 1), more than one block
    assert [(-n) % HR.WPB for n in HR.ROW_COUNTS] == [3, 1, 0, 3, 1] and max(HR.ROW_COUNTS) == HR.N_ROWS > 2 * HR.WPB
    # slot_particle: lanes of the last pair row are idle at the odd sizes
    for N in (63, 65, 129, 257):
        ppl = HR.launch_ppl(N)
        assert 64 * ppl > N


@pytest.mark.parametrize("kind", CR.KINDS)
def test_tables_hold_what_they_list(kind):
    for N in HR.HYPO_N:
        t = HR.hypo_table(kind, N)
        r, alt, w, p = t["rows4"], t["alt_var"], t["hypo_w"], t["nullhypo"]
        store = t["bel_target"] if kind == CR.BR0 else t["bel_fixed"]
        last = len(store) - 1
        assert len(r) == HR.N_ROWS and (np.diff(r[:, 2]) < 0).any() and (np.diff(r[:, 3]) < 0).any() and (r[:, 0] != np.arange(11)).sum() >= 8
        assert ((p > 0) & (p < 1)).any() and (p == 1.0).any() and (p == 0.0).any() and len(set(p[p > 0])) >= 3      # per-row probabilities
        ident = r[:, 3] == HR.IDENT_BLOCK
        assert ident.sum() == 1 and p[ident][0] == 0.3 and (store[HR.IDENT_BLOCK] == store[HR.IDENT_BLOCK][:, :1]).all()
        if kind == CR.P3P3:
            assert (alt < 0).all() and (r[:, 1] == CR.DIR_PRIOR).any()
            assert (p[r[:, 1] == CR.DIR_PRIOR] == 0).all()
            continue
        assert (alt == last).any() and (alt < 0).any() and ((alt >= 0) & (p > 0)).any() and ((alt >= 0) & (p == 0)).any()
        assert ((alt >= 0) & (w == 0.0)).any() and ((alt >= 0) & (w == 1.0)).any()
        if kind == CR.P2P2:
            pri = r[:, 1] == CR.DIR_PRIOR
            assert pri.sum() == 1 and alt[pri][0] >= 0 and p[pri][0] == 0.0
            for d in (0, 1):
                assert ((alt >= 0) & (r[:, 1] == d)).any() and ((p > 0) & (r[:, 1] == d)).any()
            th = t["bel_fixed"][:, 2]
            assert N < 63 or (np.abs(th) > math.pi).any()                       # a block stored beyond ±π: the start point is made canonical
            straddle = [(np.cos(b) < 0).all() and (np.sin(b) > 0).any() and (np.sin(b) < 0).any() for b in th] if N > 2 else [True]
            assert any(straddle)
            for b in th:                                                          # spread under π/2 about any member
                assert np.abs(CR._np_remainder(b - b[0])).max() < math.pi / 2
        ref = HR.reference(kind, N)
        ft = ref.frac_target
        assert ft.sum() >= 3 and ((ref.nh[ft] >= HR.SPREAD_NH * 5.0) & (ref.nh[ft] <= HR.SPREAD_NH * 30.0)).all(), ref.nh   # means 5-30 m apart
        if kind == CR.P2P2 and N >= 63:                                           # the hypothesis entropy carries headings well past ±π
            e = ref.nh[:, None] * (ref.u_mh[..., 2] - 0.5)
            assert (np.abs(ref.start[..., 2] + e)[ref.unsel] > math.pi + 1.0).any()
            assert ref.frac_fixed.sum() >= 3


@pytest.mark.parametrize("kind", CR.KINDS)
def test_np_against_mp_on_every_table(kind):
    worst = {}
    for N in HR.HYPO_N:
        ref = HR.reference(kind, N)
        fig = {"root_t": ref.base.dev["t"], "root_r": ref.base.dev["r"], "ent_t": ref.dev["t"], "ent_r": ref.dev["r"], **ref.stat_dev}
        print("HYPOREF cpu %s N=%d (eps) " % (CR.NAMES[kind], N) + " ".join("%s %.2f" % (k, v / CR.EPS) for k, v in fig.items())
              + " | stat_rel %.3e stat_rel_mh %.3e entropy particles %d zone share %.3f" % (ref.stat_rel, ref.stat_rel_mh, ref.entropy.sum(), ref.zone_share))
        for k, v in fig.items():
            # np against mp: under 8 eps.  The statistic in its two summation orders is a MEASUREMENT (hypo_ref's bound takes 8 x the
            # larger); what is held here is that it stays a rounding figure: a sequential sum of N terms walks ~ sqrt(N) eps / 2, and the
            # one-pass variance amplifies that by sum d^2 / ((N - 1) var) <= ~3 on these tables
            ceiling = DEV_CEILING if k in ("root_t", "root_r", "ent_t", "ent_r") else max(8.0, 2.0 * math.sqrt(N)) * CR.EPS
            assert v <= ceiling, (N, k, v / CR.EPS)
            worst[k] = max(worst.get(k, 0.0), v)
        assert ref.rel_bound == {"t": CR.ULP64, "r": CR.ULP64} and ref.base.rel_bound == {"t": CR.ULP64, "r": CR.ULP64}
        assert CR.ULP64 <= ref.stat_rel <= 8.0 * max(8.0, 2.0 * math.sqrt(N)) * CR.EPS and CR.ULP64 <= ref.stat_rel_mh <= 8.0 * ref.stat_rel
        for v in ref.ref.values():
            assert np.isfinite(v).all()
        # the snap-zone share is what the docstring says: 0, with a wide margin, on every table
        assert ref.zone_share == 0.0 and not ref.base.zone.any()
        if kind == CR.P3P3:
            assert ref.to_pi.min() >= HR.ZONE_CLEAR, (N, ref.to_pi.min())
            q = ref.base.root["q"]
            assert (2.0 * np.arctan2(np.abs(q[..., 0]), np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1)))).min() >= HR.ZONE_CLEAR
        if kind == CR.P2P2:
            assert HR.headings_in_range(ref.ref["th"][ref.entropy])
        # what the table exercises
        t = ref.table
        p = t["nullhypo"]
        if N >= 63:
            assert (ref.null[p == 1.0]).all() and not ref.null[p == 0.0].any()
            mid = (p > 0) & (p < 1)
            assert ref.null[mid].any(axis=1).all() and not ref.null[mid].all(axis=1).any()
            if kind != CR.P3P3:
                assert (ref.null & ref.unsel).any()                             # both, in that order
                assert not ref.primary[ref.has_alt & (t["hypo_w"] == 0.0)].any() and ref.primary[t["hypo_w"] == 1.0].all()
        ident = np.nonzero(t["rows4"][:, 3] == HR.IDENT_BLOCK)[0][0]
        assert ref.sd[ident] == 0.0 and ref.sd_used[ident] == (1.0 if N > 1 else 0.0)
        if N == 1:
            assert not ref.hw_null.any()                                        # no entropy at N = 1
    print("HYPOREF cpu %s worst (eps) " % CR.NAMES[kind] + " ".join("%s %.2f" % (k, v / CR.EPS) for k, v in worst.items()))


def _oracle_variant(t, p):
    """the table as the oracle can express it: one nullhypo for every row, no prior row"""
    v = dict(t)
    v["rows4"] = t["rows4"].copy()
    v["rows4"][v["rows4"][:, 1] == CR.DIR_PRIOR, 1] = 0
    v["nullhypo"] = np.full_like(t["nullhypo"], p)
    return v


@pytest.mark.parametrize("p", (0.0, 0.3))
@pytest.mark.parametrize("kind", (CR.P2P2, CR.BR0))
def test_reference_against_the_oracle(kind, p):
    """ties the stream and tag conventions to ro_conv_*: the same particles are selected, every value is within the bounds, and every
    heading either side stores lies in (-π, π]"""
    import oracle as ro
    for N in ORACLE_N:
        t = _oracle_variant(HR.hypo_table(kind, N), p)
        ref = HR.HypoReference(t)
        r = t["rows4"]
        o = ro.make_opts(N=N, solver=ro.SOLVER_CLOSED_FORM, seed=t["seed"], stream_offset=t["stream_offset"], nullhypo=p, spread_nh=HR.SPREAD_NH)
        if kind == CR.P2P2:
            out = ro.conv_pose2pose2(o, t["mu"], t["L"], t["bel_fixed"], r[:, 2], r[:, 3], r[:, 1], factor=r[:, 0],
                                     alt_var=t["alt_var"], hypo_w=t["hypo_w"], spread_nh=HR.SPREAD_NH)
            assert HR.headings_in_range(out[:, 2]) and HR.headings_in_range(ref.ref["th"][ref.entropy])
        else:
            out = ro.conv_pose2point2br(o, 0, t["mu"], t["L"], t["bel_fixed"], t["bel_target"], r[:, 2], r[:, 3], factor=r[:, 0],
                                        alt_var=t["alt_var"], hypo_w=t["hypo_w"], spread_nh=HR.SPREAD_NH)
        # selection, read off the oracle's values: a particle is solved iff it sits on its root (entropy moves it by metres; at N = 1
        # a null particle keeps its start point, metres from the root as well)
        bt, br = ref.bounds()
        et, er = CR.distance(kind, out, ref.base.root)
        solved = (et <= 1e-9) & (er <= 1e-9)
        assert np.array_equal(solved, ~ref.entropy), (kind, N, p, np.argwhere(solved == ref.entropy)[:4].tolist())
        fig, bad = ref.check(out)
        print("HYPOREF oracle %s N=%d p=%.1f t %.3f r %.3f of the bound, %d entropy particles" % (CR.NAMES[kind], N, p, fig["t"], fig["r"], fig["entropy"]))
        assert not bad, (kind, N, p, bad)


def test_bearing_range_towards_the_pose_geometry():
    """the rings of a row's two landmarks never intersect: against the other landmark the range residual alone exceeds 6 σ for every pose on
    the own ring, whatever the bearing"""
    for N in HR.BR1_N:
        t = HR.br1_table(N)
        primary, own, other, z = HR.br1_landmarks(t)
        f = t["rows4"][:, 0]
        sg = t["L"][f, 1][:, None]
        assert (z[..., 1] > 1.0).all() and (z[..., 1] < 3.5).all()
        gap = np.sqrt(((own - other) ** 2).sum(axis=1)) - 2.0 * z[..., 1]          # ‖l_a - l_b‖ - ρ_z is the nearest the ring comes; minus ρ_z
        has = t["alt_var"] >= 0
        assert has.sum() >= 5 and (gap[has] > 6.0 * sg[has] + 1.0).all(), gap[has].min()
        w = t["hypo_w"]
        assert not primary[has & (w == 0.0)].any() and primary[has & (w == 1.0)].all()
        mid = has & (w > 0) & (w < 1)
        assert primary[mid].any(axis=1).all() and not primary[mid].all(axis=1).any()
