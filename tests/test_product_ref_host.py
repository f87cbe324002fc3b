"""The references of tests/product_ref.py check one another on the CPU: the float64 restatement against mpmath on the mp variables of every
table kind, against the C oracle on every table (same base, same picks, outputs), the CPU conditions of the margin rule for every table,
and the launch arithmetic the tables rely on.  A float64 model of the KERNEL'S loop structure (bandwidth chunks of 32, LDS trips of 8, the
base skip, the cache switch, the bisection) shows that each off-by-one there is caught by some table.  Run with -s, it prints the
reference-side error figures recorded in product_ref's docstring; the GPU tests derive their bounds from the same objects."""
import math
import os
import re

import numpy as np
import pytest

import conv_ref as CR
import product_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CEILING = 8.0 * PR.EPS       # np against mp: a handful of correctly rounded operations per figure, relative to its scale
# The oracle is held to the kernel's own bound (64 ulp x scale) in every part but one: the D = 6 ROTATION part of an output / a mean.  Its SO(3)
# logarithm goes through acos(c) and sqrt(1 − c²), which loses 1e-16 / sin²θ of the angle: ~1e-10 rad at π − 1e-3, where the edge variables sit.
ORACLE_ROTATION_BOUND = 1e-9
TABLES = dict(PR.all_tables())


def _kind(name):
    return name.split()[0]


def _mp_names():
    return [n for n, mk in TABLES.items() if mk()["mp_vars"]]


def _dev_c():
    """dev_c per table kind, from the mp variables (cached references)"""
    dev = {}
    for n in _mp_names():
        ref = PR.reference(n, True)
        dev[_kind(n)] = max(dev.get(_kind(n), 0.0), ref.dev["c"])
    return dev


def test_launch_arithmetic_and_every_branch_is_entered():
    src = open(os.path.join(ROOT, "rome.jl_amd", "csrc", "rome_product.hip")).read()
    for name, val in (("kProdWaves", PR.PROD_WAVES), ("kProdChunk", PR.PROD_CHUNK), ("kProdMaxK", PR.PROD_MAXK), ("kProdMaxN", PR.PROD_MAXN)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == val
    for a, b, S in ((1, 64, 1), (65, 128, 2), (129, 256, 4), (257, 512, 8)):     # launch_product's N ranges
        assert PR.launch_shape(3, a, 2)["S"] == S == PR.launch_shape(3, b, 2)["S"]
    assert [PR.launch_shape(2, N, 2)["T4"] for N in (64, 128, 256, 512)] == [1, 1, 1, 2]
    # slots per lane: every S at its emptiest (N = 64·S/2 + 1 ...) and full; N = 1, 2
    for D in PR.DIMS:
        shapes = {N: PR.launch_shape(D, N, 2) for N in PR.SHAPE_N[D]}
        assert {s["S"] for s in shapes.values()} == ({1, 2, 4, 8} if D < 6 else {1, 2, 4})
        assert shapes[65]["idle"] == 63 and shapes[129]["idle"] == 127 and shapes[64]["idle"] == 0 and shapes[1]["idle"] == 63
        if D < 6:
            assert shapes[257]["idle"] == 255 and shapes[257]["T4"] == 2 and not shapes[512]["staged"]
    # chunk trips and wave dealing
    trips = {K: PR.launch_shape(3, 65, K) for K in PR.SHAPE_K + PR.LARGE_K}
    assert [trips[K]["trips"] for K in (2, 9, 10, 17, 18)] == [1, 1, 2, 2, 3]
    assert trips[10]["chunks"] == [8, 1] and trips[18]["chunks"] == [8, 8, 1] and trips[17]["chunks"] == [8, 8] and trips[9]["chunks"] == [8]
    assert {c for K in PR.SHAPE_K for c in PR.launch_shape(3, 65, K)["chunks"]} >= {1, 2, 3, 4, 5, 8}   # 1..5 proposals over four waves
    assert [trips[K]["cached"] for K in PR.LARGE_K] == [True, False, False, False]
    assert [trips[K]["bw_chunks"] for K in PR.LARGE_K] == [1, 2, 2, 3]
    # base first, in the middle (the skip index), last; in the second and third bandwidth chunk
    seen = set()
    for name, mk in TABLES.items():
        if _kind(name) in ("shape", "large") and "N=65" in name:
            t = mk()
            ref = PR.reference(name)
            for v, r in enumerate(ref.res):
                if r["K"] >= 3:
                    seen.add("first" if r["base"] == 0 else "last" if r["base"] == r["K"] - 1 else "middle")
                if r["K"] > PR.PROD_MAXK:
                    seen.add("chunk%d" % (r["base"] // PR.PROD_MAXK))
                assert r["K"] < 2 or r["base"] == t["want_base"][v], (name, v)
    assert seen >= {"first", "middle", "last", "chunk0", "chunk1", "chunk2"}, seen
    # prop_rows: a permutation with unused rows in between
    t = PR.shape_table(3, 65, PR.SILVERMAN)
    assert len(set(t["rows"])) == len(t["rows"]) < len(t["prop"]) and (np.diff(t["rows"]) < 0).any()
    assert t["stream_offset"] > 2 ** 32


@pytest.mark.parametrize("D", PR.DIMS)
def test_np_product_against_mp(D):
    modes = set()
    for name in _mp_names():
        ref = PR.reference(name, True)
        t = ref.table
        if t["D"] != D:
            continue
        modes.add((_kind(name), t["mode"]))
        for v in t["mp_vars"]:
            r, m = ref.res[v], ref.mp[v]
            assert m["base"] == r["base"] and list(r["picks"]) == m["picks"], (name, v)
            assert np.abs(np.array([[float(x) for x in row] for row in m["h"]]) / r["h"] - 1.0).max() <= DEV_CEILING
            assert np.abs(np.array([float(x) for x in m["logw"]]) - r["logw"]).max() <= DEV_CEILING * r["scale_w"] * r["K"]
        print("PRODREF cpu %-30s dev_c %.2f eps  dev_out %.2f / %.2f eps  (scale_w %.1e)" % (name, ref.dev["c"] / PR.EPS, ref.dev["t"] / PR.EPS,
                                                                                         ref.dev["r"] / PR.EPS, ref.scale_w))
        for k in ("c", "t", "r"):
            assert ref.dev[k] <= DEV_CEILING, (name, k, ref.dev[k])
    assert modes >= {("shape", PR.SILVERMAN), ("shape", PR.SUPPLIED), ("large", PR.SILVERMAN), ("large", PR.SUPPLIED), ("tie", PR.SUPPLIED),
                     ("tie", PR.SILVERMAN), ("far", PR.SUPPLIED)}


@pytest.mark.parametrize("D", PR.DIMS)
def test_margin_conditions_of_every_table(D):
    """every particle of every table is decided: min g >= 1000 δ, the base is decided (or tied bit for bit, lowest l), outputs finite and
    clear of the snap zone's edge"""
    dev_c = _dev_c()
    draws = 0
    for name, mk in TABLES.items():
        t = mk()
        if t["D"] != D:
            continue
        ref = PR.reference(name)
        delta = ref.delta(dev_c[_kind(name)])
        assert ref.gap >= PR.GAP_FACTOR * delta, (name, ref.gap, delta)
        live = [r for r in ref.res if r["K"] >= 2]
        draws += t["N"] * len(live)
        for r, (gap, equal) in zip(live, ref.lnh):
            assert equal or gap >= PR.GAP_FACTOR * PR.ULP64 * D, (name, gap)
            for el in r["out"].values():
                assert np.isfinite(el).all(), name
        tied = t.get("tied")
        if tied:
            for v, members in enumerate(tied):
                if members:
                    r = ref.res[v]
                    assert len({r["h"][l].tobytes() for l in members}) == 1 and r["base"] == min(members), (name, v)
                    assert r["lnh"][list(members)].max() == r["lnh"].min(), (name, v)
        if D == 6:
            assert ref.zone_margin >= CR.ZONE_MARGIN, (name, ref.zone_margin)
    print("PRODREF cpu D=%d: %d output particles decided, 0 excluded" % (D, draws))
    # what the special tables are listed for
    tie = PR.reference("tie D=%d" % D)
    assert (tie.res[5]["h"][1:, :PR.NT[D]] == PR.FLOOR).all() and (tie.table["bw"][tie.table["rows"]] == 0.0).any()
    assert tie.res[6]["h"][2, 0] == PR.FLOOR and tie.res[6]["base"] == 2
    for N in (1, 2):
        sm = PR.reference("tie D=%d N=%d silverman" % (D, N))
        hs = [r["h"] for r in sm.res if r["K"] >= 2]
        assert all((h == h[0]).all() for h in hs) and (N == 2 or all((h == PR.FLOOR).all() for h in hs))
    far = PR.reference("far D=%d" % D)
    w0 = [np.exp(r["logw"] - r["logw"].max()) for r in far.res]
    assert sum(int((w == 0.0).sum()) for w in w0) > 0.5 * sum(len(w) for w in w0)   # most weights underflow to exactly 0
    assert all(len(np.unique(r["c"])) < len(r["c"]) for r in far.res) and far.scale_w > 1e5


@pytest.mark.parametrize("D", PR.DIMS)
def test_np_product_against_the_oracle(D):
    """ties the row scatter, the streams, the floor and the copy rules of np_product to ro.product: same base and picks (every particle),
    outputs within the kernel's 64-ulp bound (the D = 6 rotation part: 1e-9)"""
    import oracle as ro
    for name, mk in TABLES.items():
        t = mk()
        if t["D"] != D:
            continue
        out = ro.product(ro.make_opts(N=t["N"], seed=t["seed"], stream_offset=t["stream_offset"]), D, t["ptr"], t["rows"], t["prop"], t["bel"],
                         prop_bw=t["bw"])
        fig, bad = PR.reference(name).check(out, rel_r=ORACLE_ROTATION_BOUND if D == 6 else PR.ULP64)
        assert not bad, (name, bad)


@pytest.mark.parametrize("D", PR.DIMS)
def test_np_spread_against_mp_and_the_oracle(D):
    import oracle as ro
    worst = {"t": 0.0, "r": 0.0, "sd": 0.0}
    for N in PR.SHAPE_N[D]:
        ref = PR.stats_reference(D, N, N <= 129)
        for k in worst:
            worst[k] = max(worst[k], ref.dev[k])
            assert ref.dev[k] <= DEV_CEILING, (D, N, k, ref.dev[k])
        assert ref.zone_margin >= CR.ZONE_MARGIN, (D, N, ref.zone_margin)
        assert (ref.sd[3] == 0.0).all() and (np.abs(ref.bel[4, 0]) > 4e5).all()
        mean = np.empty((PR.STATS_V, D)); sd = np.empty((PR.STATS_V, D))
        for v in range(PR.STATS_V):
            mean[v], sd[v] = ro.belief_spread(ref.bel[v])
        fig, bad = ref.check(mean, sd, rel_r=ORACLE_ROTATION_BOUND if D == 6 else None)
        assert not bad, (D, N, bad)
    if D == 3:
        b = PR.stats_table(3, 65)
        assert b[1, 2, 0] > 3.0 and b[2, 2, 0] < -3.0 and (b[1, 2] < 0).any() and (b[2, 2] > 0).any()
    if D == 6:
        b = PR.stats_table(6, 65)
        assert (math.pi - np.sqrt((b[1:3, 3:, 0] ** 2).sum(axis=1)) < 1e-3).all()
    print("PRODREF cpu stats D=%d dev mean %.2f / %.2f eps  sd %.2f eps" % (D, worst["t"] / PR.EPS, worst["r"] / PR.EPS, worst["sd"] / PR.EPS))


# ------------------------------------------------------------------------------------------------------------ the kernel's loop structure
def kernel_model(t, v, mutate=None):
    """float64 restatement of k_product's CONTROL FLOW for one variable (K >= 2): bandwidths in chunks of kProdMaxK through reused buffers,
    the base as l0 + c, LDS trips of kProdChunk over the non-base proposals with the skip index, the cache switch, a running log-sum-exp
    in particle order, a sequential cumulative sum and the bisection.  `mutate` plants ONE off-by-one.  -> (base, picks)"""
    D, N = t["D"], t["N"]
    rv = t["rows"][t["ptr"][v]:t["ptr"][v + 1]]
    K = len(rv)
    floor = 2e-6 if mutate == "floor" else PR.FLOOR

    def bw(l):
        raw = t["bw"][rv[l]] if t["bw"] is not None else PR.silverman_factor(D, N) * PR.np_spread(t["prop"][rv[l]])["sd"]
        return np.maximum(raw, floor)
    ihbuf = np.zeros((PR.PROD_MAXK + 1, D)); lnbuf = np.zeros(PR.PROD_MAXK)      # (one spare row: what a stale index reads)
    base, best = 0, math.inf
    for l0 in range(0, K, PR.PROD_MAXK):
        cnt = min(PR.PROD_MAXK, K - l0)
        for c in range(cnt):
            h = bw(l0 + c)
            ihbuf[c] = 1.0 / h; lnbuf[c] = np.log(h).sum()
        for c in range(cnt):
            if lnbuf[c] < best:
                best, base = lnbuf[c], l0 + c
    cached = K <= PR.PROD_MAXK + (1 if mutate == "cache" else 0)
    X = t["prop"][rv[base]].T
    lw = np.zeros(N)
    last = K - 1 - (1 if mutate == "trip" else 0)                                # trip: `c0 < K - 2` drops a trip that holds one proposal
    for c0 in range(0, last, PR.PROD_CHUNK):
        cnt = min(PR.PROD_CHUNK, K - 1 - c0)
        contrib = []
        for c in range(cnt):
            nb = c0 + c
            l = nb if (nb <= base if mutate == "skip" else nb < base) else nb + 1
            l = min(l, K - 1)
            ih = ihbuf[min(l, PR.PROD_MAXK)] if cached else 1.0 / bw(l)
            d = PR.tangent_about(D, X[:, None, :], t["prop"][rv[l]].T[None, :, :]) * ih
            q = (d * d).sum(axis=-1)
            qmin, sacc = np.full(N, math.inf), np.zeros(N)
            with np.errstate(all="ignore"):
                for j in range(N):
                    dq = q[:, j] - qmin
                    e = np.exp(-0.5 * np.abs(dq))
                    sacc = np.where(dq < 0.0, sacc * e + 1.0, sacc + e)
                    qmin = np.minimum(qmin, q[:, j])
                contrib.append(-0.5 * qmin + np.log(sacc))
        for c in range(cnt):
            lw += contrib[c]
    w = np.exp(lw - lw.max())
    cum = np.zeros(N); run = 0.0
    for m in range(N):
        run += w[m]; cum[m] = run
    u = PR.uniform3(t["seed"], t["stream_offset"] + v)
    picks = []
    for i in range(N):
        tau = (i + u) * cum[-1] / N
        lo, hi = 0, N - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if cum[max(mid - 1, 0)] > tau if mutate == "bisect" else cum[mid] > tau:
                hi = mid
            else:
                lo = mid + 1
        picks.append(lo)
    return base, np.array(picks)


MUTATIONS = {"trip": "shape D=3 N=65 silverman", "skip": "shape D=2 N=65 bw", "cache": "large D=3 N=16 silverman", "floor": "tie D=2",
             "bisect": "far D=2"}


def _model_disagrees(name, mutate):
    ref = PR.reference(name)
    hit = []
    for v, r in enumerate(ref.res):
        if r["K"] >= 2:
            base, picks = kernel_model(ref.table, v, mutate)
            if base != r["base"] or not np.array_equal(picks, r["picks"]):
                hit.append(v)
    return hit


def test_kernel_order_model_agrees_and_each_off_by_one_is_caught():
    """The unmutated model -- the kernel's order of operations -- picks what np_product picks on every particle; each planted off-by-one
    (LDS trip count, base skip index, cache switch, floor, the bisection's comparison) changes a base or a pick on the table listed."""
    for name in sorted(set(MUTATIONS.values()) | {"tie D=3", "large D=2 N=16 bw", "tie D=2 N=2 silverman"}):
        assert _model_disagrees(name, None) == [], name
    for mutate, name in MUTATIONS.items():
        hit = _model_disagrees(name, mutate)
        print("PRODREF cpu off-by-one %-6s caught by %-26s variables %s" % (mutate, name, hit))
        assert hit, (mutate, name)
