"""The references of tests/kde_ref.py check one another on the CPU: the float64 restatement against mpmath on the mp subset (f, g and
the density), np_lcv and np_kde_max against the C oracle, every CPU condition that makes the comparison rules of the GPU tests total
(decision margins, single root of g, top-two gaps, mask separation, extents of the circular tables), and the launch arithmetic the
tables are chosen from.  Run with -s, it prints the figures recorded in kde_ref's docstring; the GPU tests derive their bounds from
the same objects."""
import math
import os
import re

import mpmath as mpm
import numpy as np

import kde_ref as KR
import oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CEILING = 8.0 * KR.EPS        # np against mp, relative to the figure's scale: 8·dev stays below the 64 ulp floor of every δ
TABLES = dict(KR.all_tables())
MAX_TABLES = dict(KR.all_max_tables())


def test_launch_shape_mirrors_the_dispatch_and_every_class_is_run():
    src = open(os.path.join(ROOT, "rome.jl_amd", "csrc", "rome_kde.hip")).read()
    body = src[src.index("hipError_t launch_kde_bandwidth"):]
    assert re.search(r"auto slow = \[&\]\(auto S\) \{[^{}]*hipLaunchKernelGGL\(\(k_kde_bandwidth<decltype\(S\)::value>\)", body)
    assert re.search(r"auto fast = \[&\]\(auto B\) \{[^{}]*constexpr int b = decltype\(B\)::value;\s*hipLaunchKernelGGL\(\(k_kde_bandwidth_fast<b>\)", body)
    assert body.count("hipLaunchKernelGGL") == 2                                  # each launch is written once
    chain = re.findall(r"^  (if|else if|else)(?: \(N (<|<=) (\d+)\))? (slow|fast)\(Int<(\d+)>\{\}\);$", body, re.M)
    assert [c[0] for c in chain] == ["if"] + ["else if"] * 4 + ["else"] and body.count("Int<") == 6
    tops = [int(n) - (op == "<") for _, op, n, _, _ in chain[:-1]]               # the largest N of every class but the last
    assert tops == [7, 70, 100, 128, 256]

    def dispatched(N):                                                            # the class the chain in the source launches for N
        kind, arg = next(((k, a) for (_, _, _, k, a), top in zip(chain, tops) if N <= top), chain[-1][3:])
        return kind + arg
    for top in tops:                                                              # every dispatch edge and the class on both sides of it
        assert dispatched(top) == KR.launch_shape(top)["cls"] != KR.launch_shape(top + 1)["cls"] == dispatched(top + 1), top
    assert int(re.search(r"constexpr int kKdeWaves = (\d+);", src).group(1)) == KR.KDE_WAVES
    assert float(re.search(r"constexpr double kTieEps = ([0-9.e-]+);", src).group(1)) == KR.TIE_EPS
    assert re.search(r"nowrap = CIRC && \(yhi - ylo\) < 3\.0;", src) and KR.WRAP_EXTENT == 3.0
    cls = lambda N: KR.launch_shape(N)["cls"]
    for a, b in ((7, 8), (70, 71), (100, 101), (128, 129), (256, 257)):          # both sides of every dispatch edge are run
        assert cls(a) != cls(b) and a in KR.SHAPE_N and b in KR.SHAPE_N
    assert {cls(N) for N in KR.SHAPE_N} == {"slow1", "fast7", "fast10", "fast13", "slow4", "slow8"}
    assert {cls(N) for N in KR.CIRC_N} == {"fast7", "fast10", "fast13", "slow4"}
    fast = {N: KR.launch_shape(N) for N in KR.SHAPE_N if KR.launch_shape(N)["kernel"] == "fast"}
    assert {s["nb"] for s in fast.values()} >= {2, 3, 8, 9, 10}                  # N >= 8 with B = 7: two blocks at the least
    assert fast[8]["nb"] == 2 and fast[8]["busy"] == 3 and fast[8]["pad"] == 6 and fast[14]["pad"] == 0 and fast[15]["pad"] == 6
    assert fast[63]["pad"] == 0 and fast[64]["pad"] == 6 and fast[70]["pad"] == 0 and fast[70]["busy"] == 55 and fast[71]["pad"] == 9
    assert fast[104]["pad"] == 0 and fast[104]["nb"] == 8 and fast[105]["pad"] == 12 and fast[105]["nb"] == 9
    assert fast[100]["pad"] == 0 and fast[100]["busy"] == 55 and fast[101]["pad"] == 3 and fast[128]["pad"] == 2 and fast[128]["busy"] == 55
    for N, s in fast.items():                                                     # the staging row (136 floats) and <= 10 cells per row
        assert s["nb"] <= 10 and s["nb"] * s["B"] <= 136 and s["busy"] <= 64
    slow = {N: KR.launch_shape(N) for N in KR.SHAPE_N if KR.launch_shape(N)["kernel"] == "slow"}
    assert slow[2]["pad"] == 62 and slow[129]["pad"] == 127 and slow[256]["pad"] == 0 and slow[257]["pad"] == 255 and slow[512]["pad"] == 0
    for name, mk in TABLES.items():                                               # the last block of every launch has idle waves
        V, dim, _ = mk()["bel"].shape
        assert (V * dim) % KR.KDE_WAVES != 0, name


def _mp_subset():
    for name, v in KR.MP_TASKS:
        ref = KR.reference(name)
        for r in ref.runs[(ref.table["masks"][0], KR.DEFAULT_TOLS)]:
            if r["v"] == v:
                yield name, ref, r


def test_np_f_and_g_against_mp():
    dev_f = dev_g = 0.0
    kinds = set()
    with mpm.workdps(KR.DPS):
        for name, ref, r in _mp_subset():
            L = r["lik"]
            h = r["hstar"] if "1" not in r["rules"] else r["lcv"]["h"]
            mf, mts, mnh = KR.mp_fg(L.x, L.circ, h)
            ts, nh = L.g_parts(h)
            fv, fscale = L.fs(h)
            ef = abs(float(KR._f(fv) - mf)) / fscale
            eg = abs(float((KR._f(ts) - KR._f(nh)) - (mts - mnh))) / max(1.0, float(mnh), float(mts))
            print("KDEREF cpu %-24s k %d %-6s N %-3d h %.6g  dev_f %.2f eps  dev_g %.2f eps" % (name, r["k"], "circ" if L.circ else "euclid", L.N, h,
                                                                                             ef / KR.EPS, eg / KR.EPS))
            dev_f, dev_g = max(dev_f, ef), max(dev_g, eg)
            kinds.add((KR.family(name), KR.launch_shape(L.N)["cls"], L.circ))
    print("KDEREF cpu dev_f %.2f eps  dev_g %.2f eps" % (dev_f / KR.EPS, dev_g / KR.EPS))
    assert dev_f <= DEV_CEILING and dev_g <= DEV_CEILING
    assert {c for f, c, _ in kinds if f == "shape"} == {"slow1", "fast7", "fast10", "fast13", "slow4", "slow8"}
    assert {f for f, _, _ in kinds} == {"shape", "circ", "mask", "outlier", "wide", "degenerate"}


def test_np_density_against_mp():
    dev = 0.0
    with mpm.workdps(KR.DPS):
        for name, v in KR.MP_MAX_TASKS:
            ref = KR.max_reference(name)
            t = ref.table
            for k in range(3):
                r = ref.res[3 * v + k]
                my = KR.mp_kde_density(t["bel"][v, k], t["bw"][v, k], r["grid"])
                assert max(range(t["G"]), key=lambda g: (my[g], -g)) == r["g"]
                e = max(abs(float(KR._f(a) - b)) for a, b in zip(r["y"], my)) / r["scale"]
                dev = max(dev, e)
    print("KDEREF cpu dev_y %.2f eps" % (dev / KR.EPS))
    assert dev <= DEV_CEILING


def test_cpu_conditions_of_every_table_and_the_tie_band():
    """rule 1: every decision margin >= 1000 δ_f; rule 3: one + to − root of g on the extended bracket; every task has a rule"""
    worst, decisions, ties, tasks = math.inf, 0, 0, 0
    for name in TABLES:
        ref = KR.reference(name)
        assert not ref.failures(), (name, ref.failures()[:4])
        for (mask, tols), rs in ref.runs.items():
            assert len(rs) == ref.V * ref.dim
            for r in rs:
                tasks += 1
                assert r["rules"] in (("1", "2"), ("2",), ("3",)) and math.isfinite(r["hstar"]) and r["hstar"] > 0
                if "1" in r["rules"]:
                    worst = min(worst, r["margin"])
                    decisions += len(r["lcv"]["margins"])
                    if KR.launch_shape(ref.N)["kernel"] == "fast":
                        ties += sum(1 for m in r["lcv"]["margins"] if m[0] < KR.TIE_EPS)
        if ref.table["wide"]:                                                     # excused from rule 1, decided by rule 2
            assert all(r["rules"] == ("2",) for rs in ref.runs.values() for r in rs)
    print("KDEREF cpu %d tasks, %d rule-1 decisions, smallest margin %.3g δ_f, %d fast-path decisions inside kTieEps; reseeded: %s" % (
        tasks, decisions, worst, ties, KR.RESEED))
    assert worst >= KR.GAP_FACTOR and ties >= 20


def test_a_wrong_decision_inside_the_tie_band_breaks_rule_1():
    """what rule 1 pins: with ONE reference decision inside kTieEps taken the other way -- a single-precision comparison that was not
    re-decided in double -- the answer leaves the 64 ulp window by orders of magnitude, or the search comes back to the same point
    within an ulp (the golden section reuses its interior points: the two brackets share the point next to a near-tie)"""
    planted, caught, least = 0, 0, math.inf
    for name in TABLES:
        ref = KR.reference(name)
        if KR.launch_shape(ref.N)["kernel"] != "fast":
            continue
        for (mask, tols), rs in ref.runs.items():
            for r in rs:
                if "1" not in r["rules"]:
                    continue
                for i, m in enumerate(r["lcv"]["margins"]):
                    if m[0] < KR.TIE_EPS:
                        h = KR.np_lcv(None, r["circ"], r["tol"], r["lik"], flip=i)["h"]
                        planted += 1
                        e = abs(h / r["lcv"]["h"] - 1.0)
                        if e > KR.ULP64:
                            caught += 1
                            least = min(least, e)
                        else:
                            assert e <= 2.0 * KR.EPS
    print("KDEREF cpu %d planted tie decisions: %d leave the rule-1 window, by >= %.3g" % (planted, caught, least))
    assert caught >= 20 and least > 1000.0 * KR.ULP64


def test_np_lcv_against_the_oracle():
    """under the rule-1 condition the golden-section iterates are the oracle's: 64 ulp"""
    worst = 0.0
    for name in TABLES:
        ref = KR.reference(name)
        for (mask, tols), rs in ref.runs.items():
            if not any("1" in r["rules"] for r in rs):
                continue
            ho = ro.kde_bandwidths(ref.table["bel"], mask, *tols).reshape(-1)
            for r, h in zip(rs, ho):
                if "1" in r["rules"]:
                    e = abs(h / r["lcv"]["h"] - 1.0)
                    worst = max(worst, e)
                    assert e <= KR.ULP64, (name, mask, tols, r["v"], r["k"], h, r["lcv"]["h"])
    print("KDEREF cpu np_lcv against the oracle: %.2f eps" % (worst / KR.EPS))
    eq = KR.reference("degenerate equal")
    for r in eq.runs[(0, KR.DEFAULT_TOLS)]:                                      # minm = 1e-6 and f monotone in h: the search runs to the left end
        assert r["lik"].bracket() == (1e-6, 1e-6) and 0 < r["lcv"]["h"] <= 1e-5 and r["lik"].f(1e-7) < r["lik"].f(1e-6) < r["lik"].f(1e-5)


def test_mask_tables_separate_the_two_treatments():
    """every coordinate of every mask table: the circular and the Euclidean reference bandwidth differ by > 100 x the bound applied"""
    least = math.inf
    for name in TABLES:
        if KR.family(name) != "mask":
            continue
        ref = KR.reference(name)
        (m0, r0), (m1, r1) = [(mask, rs) for (mask, _), rs in ref.runs.items()]
        assert m0 ^ m1 == (1 << ref.dim) - 1
        for a, b in zip(r0, r1):
            assert a["circ"] != b["circ"]
            bound = max(KR.ULP64 if "1" in r["rules"] else r["tol"] if "3" in r["rules"] else 2 * r["tol"] / (1 - 2 * r["tol"]) for r in (a, b))
            ha, hb = (r["lcv"]["h"] if "1" in r["rules"] else r["hstar"] for r in (a, b))
            least = min(least, abs(ha / hb - 1.0) / bound)
    print("KDEREF cpu mask tables: circular and Euclidean bandwidths differ by >= %.3g bounds" % least)
    assert least > 100.0


def test_circular_tables_run_the_nowrap_route_and_the_wrapped_body():
    for N in KR.CIRC_N:
        t = KR.circ_table(N)
        ext = np.array([[KR.Lik(t["bel"][v, k], True).extent() for k in range(3)] for v in range(t["bel"].shape[0])])
        assert (ext[:, 0] < KR.WRAP_EXTENT).all() and (ext[:, 1:] >= KR.WRAP_EXTENT).all(), (N, ext)
        assert (np.abs(t["bel"]) <= math.pi).all()
    for N in KR.SHAPE_N:                                                          # the heading beliefs straddle ±π and stay concentrated
        x = KR.shape_table(N)["bel"][:, 2]
        assert (np.abs(x) > 2.5).all() and (N < 8 or ((x.max(axis=1) > 3.0) & (x.min(axis=1) < -3.0)).any())
        assert max(KR.Lik(b, True).extent() for b in x) < KR.WRAP_EXTENT


def test_np_kde_max_against_the_oracle_and_the_gap_condition():
    least, pairs = math.inf, set()
    for name in MAX_TABLES:
        ref = KR.max_reference(name)
        t = ref.table
        mo = ro.kde_max(t["bel"], t["bw"], t["G"]).reshape(-1)
        for r, X in zip(ref.res, mo):
            assert abs(X - r["X"]) <= KR.ULP64 * max(1.0, abs(r["lo"]), abs(r["hi"])), (name, X, r["X"])
        assert (t["bel"].shape[0] * 3 == 48) == (t["key"][1] == "pair")
        if t["key"][1] == "zero":                                                # every density value is 0: the first grid point, lo
            assert all(r["g"] == 0 and r["gap"] == math.inf and not r["y"].any() for r in ref.res)
            continue
        assert ref.gap >= KR.GAP_FACTOR, (name, ref.gap)
        least = min(least, ref.gap)
        pairs.add(t["key"][2:])
        if t["key"][1] == "narrow":
            assert all(abs(h / (r["step"] / 4.0) - 1.0) < 1e-12 for r, h in zip(ref.res, t["bw"].reshape(-1)))
    print("KDEREF cpu kde_max: smallest top-two gap %.3g δ_y" % least)
    assert {G for _, G in pairs} >= {2, 3, 63, 64, 65, 128, 129, 192, 193, 255, 256} and {N for N, _ in pairs} == {3, 63, 64, 65, 512}
    hit = {r["g"] == t_G - 1 for name in MAX_TABLES for t_G in [KR.max_reference(name).table["G"]] for r in KR.max_reference(name).res}
    assert hit == {False, True}                                                   # g = G − 1 (-> hi) is some task's answer
