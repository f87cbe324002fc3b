"""References for stage 2 of the partial-aware product (k_product_coord<S>, rome.jl_amd/csrc/rome_product_partial.hip): what
rome_product_partial_dev / rome_product_partial must leave in `bel` for every particle of every line.  The definition is DESIGN.md §12d.

Two sides, neither of which is the kernel:
  * mp_task -- mpmath at lin_ref.DPS digits, one task.
  * np_task -- float64 NumPy, written the plain way and NOT in the kernel's order: two-pass spread, max-shifted log-sum-exp over all N kernel
               points at once, np.cumsum, np.searchsorted(c, τ, "right") clipped to N − 1.

Definition restated.  Task (v, c): densities l = 0 .. M − 1 = the lines prop[r][c][0..N) of its rows r in order, then (joint) bel[v][c][0..N).
M = 1: the output line is that density, bit for bit.  M >= 2: h_l = max(bw_l, 1e-6), bw_l supplied (prop_bw[r][c] / joint_bw[v][c]) or
Silverman's c_N·sd_l, c_N = (4/(3N))^(1/5), sd_l the sample std (divisor N − 1; N = 1: 1) of the differences about point 0 (wrapped to
(−π, π] on a circular coordinate).  Base b = the smallest h_l, ties to the lowest l.  log w_i = Σ_{l≠b} log Σ_j exp(−½ (d(x_bi, x_lj)/h_l)²).
One uniform u = (w₀ + ½)/2³² from Philox counter (0xFFFFFFFF, stream, 3 << 16), stream = stream_offset + v·D + c; output particle i picks the
first m with c_m > (i + u)/N (c: normalised cumulative weights), else N − 1, and is x_bm + h_p·ξ_i, 1/h_p² = Σ_l 1/h_l², ξ_i =
ro.rng_normals(seed, stream, i, 1), wrapped on a circular coordinate.  Lines without a task are J's, bit for bit.

Comparison rule (the one of product_ref.py, every particle decided, none left out).  For output particle i the reference alone evaluates the
margin g_i = min_m |(i + u)/N − c_m| over the distinct values of its c (the last one left out: it decides no pick).  δ = max(8·dev_c, 64 ulp)
x scale_w, scale_w = max(1, largest |log-weight term| of the task).  CONDITIONS, checked on the CPU (tests/test_partial_product_host.py):
every task has min_i g_i >= 1000·δ, and its two smallest h are bit-equal by construction or >= 1000·64 ulp apart (relative).  A table that
misses one gets another seed (RESEED).  On the GPU:
  * the pick of every particle, recovered from out − h_p·ξ as the nearest base point (which must lie within the output bound), equals the
    reference's -- up to base points that are bit-equal to one another, which no output can tell apart;
  * out = x_b[pick] + h_p·ξ within max(8·dev_out, 64 ulp) x max(1, largest |coordinate| of the task's densities), wrapped on circular
    coordinates;
  * M = 1 lines and lines without a task are bit copies.

Measured dev (CPU, np against mp, printed by tests/test_partial_product_host.py -s), in units of eps = 2^-52:
  dev_c <= 0.51   dev_out <= 0.47   (shape, zero-spread, far-apart and tie tables, D = 2 / 3 / 6; 88 mp tasks)
Every 8·dev lies below the floor, so every bound is the floor, 64 ulp = 1.42e-14 times its scale; the host test holds every dev under 8 eps.
"""
import functools
import math

import mpmath as mpm
import numpy as np

from lin_ref import DPS, EPS, _wrap
from product_ref import FLOOR, GAP_FACTOR, ULP64, _remainder, uniform3

SEED = 0x50415254
DIMS = (2, 3, 6)
CIRC = {2: 0, 3: 0b100, 6: 0b111000}
SILVERMAN, SUPPLIED = "silverman", "bw"
MODES = (SILVERMAN, SUPPLIED)
SHAPE_N = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512)
MP_SHAPE_N = 65
MAXN = 512                                                  # kCoordMaxN

# per D: (joint, ((cover, rows), ...)) of every variable.  M runs over 1, 2, 3, 9 with and without the joint density; every D has a
# variable with two or more tasks and lines nobody covers, one with no task at all, Euclidean and (D = 3, 6) circular tasks
LAYOUT = {
    6: ((0, (((0, 1, 5), 2),)),                             # M = 2 on x, y, ω_z; z, ω_x, ω_y untouched
        (1, (((0, 1, 5), 2), ((2, 3, 4), 1))),              # joint: M = 3 and M = 2
        (0, (((2,), 1), ((3,), 9), ((5,), 3))),             # M = 1 (copy), 9, 3
        (1, (((4,), 8),)),                                  # joint: M = 9, circular
        (1, ())),                                           # no task
    3: ((0, (((0, 1), 3),)),                                # three ranges and nothing else: the heading is untouched
        (1, (((0, 1), 1), ((2,), 2))),                      # joint: M = 2, and M = 3 on the heading
        (0, (((2,), 9), ((0,), 1))),                        # M = 9 circular, M = 1 copy
        (0, ())),
    2: ((0, (((0,), 2),)),                                  # M = 2; y untouched
        (1, (((1,), 2), ((0,), 8))),                        # joint: M = 3, M = 9
        (0, (((1,), 1),)),                                  # M = 1 (copy)
        (1, ())),
}
# table key -> seed bump, for a table whose fixed seed missed a CPU condition
RESEED = {}


def silverman_factor(N):
    return (4.0 / (3.0 * N)) ** 0.2


def is_circ(t, c):
    return bool((t["circ"] >> c) & 1)


def tasks_of(ptr, rows, cover, joint, D):
    """the task tables of a layout, derived here and not by the package: per variable (CSR ptr / rows of its PARTIAL rows) and coordinate"""
    tv, tc, tp, tr, tj = [], [], [0], [], []
    for v in range(len(ptr) - 1):
        for c in range(D):
            cov = [r for r in rows[ptr[v]:ptr[v + 1]] if c in cover[r]]
            if cov:
                tv.append(v); tc.append(c); tj.append(joint[v]); tr += cov; tp.append(len(tr))
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return {"task_var": i32(tv), "task_coord": i32(tc), "task_ptr": i32(tp), "task_rows": i32(tr), "task_joint": i32(tj)}


def densities(t, k):
    """-> (list of (N,) lines, list of supplied bandwidths or Nones) of task k, in the order of the definition"""
    tk = t["tasks"]
    v, c = int(tk["task_var"][k]), int(tk["task_coord"][k])
    rows = tk["task_rows"][tk["task_ptr"][k]:tk["task_ptr"][k + 1]]
    dens = [t["prop"][r, c] for r in rows]
    bws = [None if t["bw"] is None else t["bw"][r, c] for r in rows]
    if tk["task_joint"][k]:
        dens.append(t["bel"][v, c])
        bws.append(None if t["jbw"] is None else t["jbw"][v, c])
    return dens, bws


def stream_of(t, k):
    return t["stream_offset"] + int(t["tasks"]["task_var"][k]) * t["D"] + int(t["tasks"]["task_coord"][k])


def normals1(seed, stream, N):
    import oracle as ro
    return np.array([ro.rng_normals(seed, stream, i, 1)[0] for i in range(N)])


# ------------------------------------------------------------------------------------------------------------ float64 side
def _diff(circ, a, b):
    return _remainder(a - b) if circ else a - b


def np_bandwidth(x, bw, circ):
    if bw is not None:
        return max(float(bw), FLOOR)
    d = _diff(circ, x, x[0])
    e = d - d.mean()
    return max(silverman_factor(len(x)) * math.sqrt(float((e * e).sum()) / max(len(x) - 1, 1)), FLOOR)


def np_task(t, k, xi=None):
    """M >= 2: base, h (M,), hp, terms (M − 1, N), logw, c, u, tau, picks, out (N,), scales; M = 1: {"M": 1, "src": the line to copy}"""
    N = t["N"]
    c = int(t["tasks"]["task_coord"][k])
    circ = is_circ(t, c)
    dens, bws = densities(t, k)
    M = len(dens)
    if M == 1:
        return {"M": 1, "src": dens[0]}
    h = np.array([np_bandwidth(x, b, circ) for x, b in zip(dens, bws)])
    base = int(np.argmin(h))                                                    # the first of equal minima
    X = dens[base]
    terms = []
    with np.errstate(all="ignore"):
        for l in range(M):
            if l == base:
                continue
            d = _diff(circ, X[:, None], dens[l][None, :]) / h[l]
            e = -0.5 * d * d
            mx = e.max(axis=1)
            terms.append(mx + np.log(np.exp(e - mx[:, None]).sum(axis=1)))
    terms = np.array(terms)
    logw = terms.sum(axis=0)
    w = np.exp(logw - logw.max())
    cum = np.cumsum(w)
    cc = cum / cum[-1]
    stream = stream_of(t, k)
    u = uniform3(t["seed"], stream)
    tau = (np.arange(N) + u) / N
    picks = np.minimum(np.searchsorted(cc, tau, side="right"), N - 1)
    hp = 1.0 / math.sqrt(float((1.0 / (h * h)).sum()))
    if xi is None:
        xi = normals1(t["seed"], stream, N)
    return {"M": M, "base": base, "h": h, "hp": hp, "terms": terms, "logw": logw, "c": cc, "u": u, "tau": tau, "picks": picks, "xi": xi,
            "out": X[picks] + hp * xi, "X": X, "circ": circ, "scale_w": max(1.0, float(np.abs(terms).max())),
            "scale_x": max(1.0, max(float(np.abs(x).max()) for x in dens))}


def pick_gap(r):
    """min_i g_i of one task (product_ref.pick_gap on its c)"""
    cv = np.unique(r["c"][:-1])
    if len(cv) == 0:
        return math.inf
    j = np.clip(np.searchsorted(cv, r["tau"]), 1, len(cv) - 1) if len(cv) > 1 else np.zeros(len(r["tau"]), int)
    lo = np.abs(r["tau"] - cv[np.maximum(j - 1, 0)])
    return float(np.minimum(lo, np.abs(r["tau"] - cv[j])).min())


def h_gap(r):
    """(relative gap between the two smallest h, whether they are bit-equal)"""
    s = np.sort(r["h"])
    return float((s[1] - s[0]) / s[0]), bool(s[1] == s[0])


# ------------------------------------------------------------------------------------------------------------ mpmath side
def _f(v):
    return mpm.mpf(float(v))


def mp_task(t, k, xi):
    """one task (M >= 2) at the current mp precision -> base, h, hp, logw, c, picks, out"""
    N = t["N"]
    c = int(t["tasks"]["task_coord"][k])
    circ = is_circ(t, c)
    dens, bws = densities(t, k)
    dens = [[_f(x) for x in line] for line in dens]
    M = len(dens)
    diff = (lambda a, b: _wrap(a - b)) if circ else (lambda a, b: a - b)
    cn = (mpm.mpf(4) / (3 * N)) ** (mpm.mpf(1) / 5)
    h = []
    for x, b in zip(dens, bws):
        if b is not None:
            raw = _f(b)
        else:
            d = [diff(a, x[0]) for a in x]
            md = sum(d) / N
            raw = cn * mpm.sqrt(sum((a - md) ** 2 for a in d) / max(N - 1, 1))
        h.append(max(raw, _f(FLOOR)))
    base = min(range(M), key=lambda l: (h[l], l))
    logw = []
    for i in range(N):
        acc = mpm.mpf(0)
        for l in range(M):
            if l != base:
                acc += mpm.log(sum(mpm.exp(-(diff(dens[base][i], y) / h[l]) ** 2 / 2) for y in dens[l]))
        logw.append(acc)
    mx = max(logw)
    w = [mpm.exp(x - mx) for x in logw]
    tot = sum(w)
    cc, run = [], mpm.mpf(0)
    for x in w:
        run += x
        cc.append(run / tot)
    u = _f(uniform3(t["seed"], stream_of(t, k)))                                # u is a double by definition
    picks = [next((m for m in range(N) if cc[m] > (i + u) / N), N - 1) for i in range(N)]
    hp = 1 / mpm.sqrt(sum(1 / (x * x) for x in h))
    out = [dens[base][picks[i]] + hp * _f(xi[i]) for i in range(N)]
    return {"base": base, "h": h, "hp": hp, "logw": logw, "c": cc, "picks": picks, "out": out, "circ": circ}


# ------------------------------------------------------------------------------------------------------------ tables
def _line(rng, N, centre, sigma, circ, bimodal=False):
    x = centre + 0.5 * sigma * rng.standard_normal() + sigma * rng.standard_normal(N)
    if bimodal:
        x[::2] += 4.0 * sigma
    return np.arctan2(np.sin(x), np.cos(x)) if circ else x


def _assemble(D, N, layout, seed, stream_offset, mode, rng, fill, n_unused=2):
    """layout: per variable (joint, ((cover, n_rows), ...)).  Rows are scattered over `prop` by a random permutation among unused rows; the
    lines of a partial row OUTSIDE its cover are NaN: nobody may read them.  fill(v, c, kind, l) -> (line, supplied bandwidth) for density
    l of task (v, c) (kind "row") or for the joint line (kind "joint")."""
    V = len(layout)
    n_rows = sum(n for _, groups in layout for _, n in groups)
    R_ = n_rows + n_unused
    perm = rng.permutation(R_).astype(np.int32)
    prop = rng.standard_normal((R_, D, N)) * 3.0                                 # unused rows hold ordinary finite data
    bel = rng.standard_normal((V, D, N)) * 2.0
    bw, jbw = np.abs(rng.standard_normal((R_, D))) + 0.1, np.abs(rng.standard_normal((V, D))) + 0.1
    ptr, rows, cover, joint, at = [0], [], {}, [], 0
    for v, (jn, groups) in enumerate(layout):
        joint.append(int(jn))
        for cov, n in groups:
            for _ in range(n):
                r = int(perm[at]); at += 1
                rows.append(r); cover[r] = tuple(cov)
                prop[r] = np.nan
        ptr.append(len(rows))
    count = {}
    for v, (jn, groups) in enumerate(layout):
        for r in rows[ptr[v]:ptr[v + 1]]:
            for c in cover[r]:
                l = count.get((v, c), 0); count[(v, c)] = l + 1
                prop[r, c], bw[r, c] = fill(v, c, "row", l)
        if jn:
            for c in sorted({c for cov, _ in groups for c in cov}):
                bel[v, c], jbw[v, c] = fill(v, c, "joint", count[(v, c)])
    return {"D": D, "N": N, "V": V, "prop": prop, "bel": bel, "bw": bw if mode == SUPPLIED else None, "jbw": jbw if mode == SUPPLIED else None,
            "circ": CIRC[D], "seed": seed, "stream_offset": stream_offset, "mode": mode, "tasks": tasks_of(ptr, rows, cover, joint, D),
            "cover": cover, "joint": joint, "n_rows": R_}


def _seed(key):
    kind, D, N = key[0], key[1], key[2]
    return 9000 + 131 * DIMS.index(D) + 17 * N + 1009 * RESEED.get(key, 0) + {"shape": 0, "zero": 1, "far": 2, "tie": 3}[kind] * 100003 \
        + (50021 if key[3] == SUPPLIED else 0)


@functools.lru_cache(maxsize=None)
def shape_table(D, N, mode):
    """LAYOUT[D] at one N: per (v, c) a cluster of densities about one centre (even variables: circular clusters across ±π), one of them
    five times tighter than the others (the base: first, middle, last or the joint line in turn), every third bimodal"""
    key = ("shape", D, N, mode)
    rng = np.random.default_rng(_seed(key))
    cn = silverman_factor(N)
    centre, tight = {}, {}
    n_of = {(v, c): n + jn for v, (jn, groups) in enumerate(LAYOUT[D]) for c in range(D) for n in [sum(m for cov, m in groups if c in cov)]}

    def fill(v, c, kind, l):
        circ = bool((CIRC[D] >> c) & 1)
        if (v, c) not in centre:
            centre[(v, c)] = (math.pi - 0.05 * rng.uniform() if v % 2 == 0 else rng.uniform(-2.5, 2.5)) if circ else rng.uniform(-100, 100)
            tight[(v, c)] = int(rng.integers(0, 1 << 20)) % n_of[(v, c)]          # the tight density: any position, the joint line included
        s = (0.15 if circ else 1.0) * rng.uniform(0.7, 1.5) * (0.2 if l == tight[(v, c)] else 1.0)
        return _line(rng, N, centre[(v, c)], s, circ, bimodal=(l % 3 == 1)), cn * s * rng.uniform(0.8, 1.2)

    t = _assemble(D, N, LAYOUT[D], SEED + N, (1 << 32) + 777 if N == 65 else 500 + N, mode, rng, fill)
    t["key"] = key
    t["mp_tasks"] = [k for k in range(len(t["tasks"]["task_var"])) if 2 <= _n_dens(t, k) <= 3] if N == MP_SHAPE_N else []
    return t


def _n_dens(t, k):
    tk = t["tasks"]
    return int(tk["task_ptr"][k + 1] - tk["task_ptr"][k] + tk["task_joint"][k])


SPECIAL_N = 24
# three variables, a Euclidean and (D >= 3) a circular task each: M = 2 without the joint line, M = 2 and M = 3 with it
SPECIAL_LAYOUT = {6: ((0, (((2,), 2), ((5,), 2))), (1, (((2,), 1), ((4,), 1))), (1, (((0,), 2), ((3,), 2)))),
                  3: ((0, (((0,), 2), ((2,), 2))), (1, (((1,), 1), ((2,), 1))), (1, (((0,), 2), ((2,), 2)))),
                  2: ((0, (((0,), 2), ((1,), 2))), (1, (((1,), 1), ((0,), 1))), (1, (((0,), 2), ((1,), 2))))}


@functools.lru_cache(maxsize=None)
def zero_table(D, N=SPECIAL_N):
    """Silverman's rule on a density WITHOUT spread (every point the same double: the z = 0 that both XYYaw proposals of the chain repeat):
    sd = 0 in any arithmetic, h = the 1e-6 floor, so it is the base; density 0 of every task is such a line, the others have unit spread"""
    key = ("zero", D, N, SILVERMAN)
    rng = np.random.default_rng(_seed(key))
    centre = {}

    def fill(v, c, kind, l):
        circ = bool((CIRC[D] >> c) & 1)
        if (v, c) not in centre:
            centre[(v, c)] = rng.uniform(-2.5, 2.5) if circ else float(np.round(rng.uniform(-8, 8)))
        if l == 0:
            return np.full(N, centre[(v, c)]), 1.0
        return _line(rng, N, centre[(v, c)], 0.1, circ), 1.0

    t = _assemble(D, N, SPECIAL_LAYOUT[D], SEED + 3000, 13000, SILVERMAN, rng, fill)
    t["key"], t["mp_tasks"], t["want_base"] = key, list(range(len(t["tasks"]["task_var"]))), 0
    return t


FAR = 1000.0


@functools.lru_cache(maxsize=None)
def far_table(D, N=SPECIAL_N):
    """supplied bandwidths h; density l sits l·1000·h from density 0 and has spread 2 h: without the running maximum every weight
    underflows; the last density has the smallest bandwidth and is the base"""
    key = ("far", D, N, SUPPLIED)
    rng = np.random.default_rng(_seed(key))
    centre = {}
    n_of = {(v, c): n + jn for v, (jn, groups) in enumerate(SPECIAL_LAYOUT[D]) for cov, n in groups for c in cov}

    def fill(v, c, kind, l):
        circ = bool((CIRC[D] >> c) & 1)
        hb = 1e-4 if circ else 1e-2                                               # (circular: 1000 h = 0.1 rad apart, across ±π for v = 0)
        if (v, c) not in centre:
            centre[(v, c)] = (math.pi - 0.03 if v == 0 else rng.uniform(-2.5, 2.5)) if circ else rng.uniform(-100, 100)
        x = centre[(v, c)] + l * FAR * hb + 2.0 * hb * rng.standard_normal(N)
        return (np.arctan2(np.sin(x), np.cos(x)) if circ else x), hb * (0.5 if l == n_of[(v, c)] - 1 else 1.0 + 0.1 * l)

    t = _assemble(D, N, SPECIAL_LAYOUT[D], SEED + 4000, 14000, SUPPLIED, rng, fill)
    t["key"], t["mp_tasks"], t["want_base"] = key, list(range(len(t["tasks"]["task_var"]))), "last"
    return t


@functools.lru_cache(maxsize=None)
def tie_table(D, N=SPECIAL_N):
    """supplied bandwidths, bit-identical for EVERY density of a task (different points): the lowest l = 0 must become the base, also when
    the joint line -- the last density -- ties with the rows"""
    key = ("tie", D, N, SUPPLIED)
    rng = np.random.default_rng(_seed(key))
    centre = {}

    def fill(v, c, kind, l):
        circ = bool((CIRC[D] >> c) & 1)
        if (v, c) not in centre:
            centre[(v, c)] = rng.uniform(-2.5, 2.5) if circ else rng.uniform(-100, 100)
        s = 0.15 if circ else 1.0
        return _line(rng, N, centre[(v, c)], s, circ), 0.4 * s

    t = _assemble(D, N, SPECIAL_LAYOUT[D], SEED + 5000, 15000, SUPPLIED, rng, fill)
    t["key"], t["mp_tasks"], t["want_base"] = key, list(range(len(t["tasks"]["task_var"]))), 0
    return t


def all_tables():
    """(name, maker) of every table, built lazily"""
    for D in DIMS:
        for mode in MODES:
            for N in SHAPE_N:
                yield "shape D=%d N=%d %s" % (D, N, mode), functools.partial(shape_table, D, N, mode)
        yield "zero D=%d" % D, functools.partial(zero_table, D)
        yield "far D=%d" % D, functools.partial(far_table, D)
        yield "tie D=%d" % D, functools.partial(tie_table, D)


class Reference:
    """Everything the tests need about one table, computed once and never modified: np_task of every task, the margins, mp_task of the mp
    tasks (with_mp) and the reference's own error."""

    def __init__(self, t, with_mp=False):
        self.table = t
        self.T = len(t["tasks"]["task_var"])
        self.res = [np_task(t, k) for k in range(self.T)]
        live = [r for r in self.res if r["M"] >= 2]
        self.scale_w = max([1.0] + [r["scale_w"] for r in live])
        self.gaps = [(pick_gap(r), r["scale_w"]) for r in live]
        self.hgap = [h_gap(r) for r in live]
        self.dev = {"c": 0.0, "out": 0.0}
        self.mp = {}
        if with_mp:
            with mpm.workdps(DPS):
                for k in t["mp_tasks"]:
                    r = self.res[k]
                    m = self.mp[k] = mp_task(t, k, r["xi"])
                    self.dev["c"] = max(self.dev["c"], max(abs(float(_f(a) - b)) for a, b in zip(r["c"], m["c"])) / r["scale_w"])
                    wrap = _wrap if r["circ"] else (lambda x: x)
                    self.dev["out"] = max(self.dev["out"], max(abs(float(wrap(_f(a) - b))) for a, b in zip(r["out"], m["out"])) / r["scale_x"])

    def conditions(self, dev_c=0.0):
        """-> list of misses of the two CPU conditions"""
        bad = []
        for k, ((g, sw), (hg, eq)) in enumerate(zip(self.gaps, self.hgap)):
            if not g >= GAP_FACTOR * max(8.0 * dev_c, ULP64) * sw:
                bad.append(("pick margin", k, g, sw))
            if not (eq or hg >= GAP_FACTOR * ULP64):
                bad.append(("h gap", k, hg))
        return bad

    def expected(self):
        """bel as the definition leaves it (V, D, N), from the float64 side"""
        t = self.table
        out = t["bel"].copy()
        for k, r in enumerate(self.res):
            v, c = int(t["tasks"]["task_var"][k]), int(t["tasks"]["task_coord"][k])
            out[v, c] = r["src"] if r["M"] == 1 else (_remainder(r["out"]) if r["circ"] else r["out"])
        return out

    def check(self, out, rel=ULP64):
        """kernel output (V, D, N) against every particle of every line -> (figures, list of failures)"""
        t = self.table
        N = t["N"]
        out = np.asarray(out)
        bad, fig = [], {"out": 0.0, "pick": 0.0}
        if not np.isfinite(out).all():
            bad.append(("not finite", np.argwhere(~np.isfinite(out))[:4].tolist()))
        tasked = np.zeros(out.shape[:2], bool)
        for k, r in enumerate(self.res):
            v, c = int(t["tasks"]["task_var"][k]), int(t["tasks"]["task_coord"][k])
            tasked[v, c] = True
            if r["M"] == 1:
                if not np.array_equal(out[v, c], r["src"]):
                    bad.append(("M = 1 line is not a bit copy", k))
                continue
            b = rel * r["scale_x"]
            with np.errstate(all="ignore"):
                e = np.abs(_diff(r["circ"], out[v, c], r["out"]))
                fig["out"] = max(fig["out"], float((e / b).max()))
                if not (e <= b).all():
                    bad.append(("output", k, np.nonzero(~(e <= b))[0][:4].tolist(), float((e / b).max())))
                if r["circ"] and not (np.abs(out[v, c]) <= math.pi + b).all():
                    bad.append(("circular output outside [-pi, pi]", k))
                # the pick, recovered from out − hp·ξ: the nearest base point, which must lie within the output bound
                cand = out[v, c] - r["hp"] * r["xi"]
                dist = np.abs(_diff(r["circ"], cand[:, None], r["X"][None, :]))
                near = dist.argmin(axis=1)
                best = dist[np.arange(N), near]
                fig["pick"] = max(fig["pick"], float((best / b).max()))
                wrong = (r["X"][near] != r["X"][r["picks"]]) | ~(best <= b)       # (bit-equal base points cannot be told apart)
                if wrong.any():
                    bad.append(("pick", k, np.nonzero(wrong)[0][:6].tolist(), near[wrong][:6].tolist(), r["picks"][wrong][:6].tolist(), float((best / b).max())))
        if not np.array_equal(out[~tasked], t["bel"][~tasked]):
            bad.append(("a line without a task is not a bit copy of J", np.argwhere(~tasked)[:4].tolist()))
        return fig, bad


@functools.lru_cache(maxsize=None)
def reference(name, with_mp=False):
    return Reference(dict(all_tables())[name](), with_mp)
