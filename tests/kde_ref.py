"""References for the KDE kernels of rome.jl_amd/csrc/rome_kde.hip: the leave-one-out likelihood bandwidths (k_kde_bandwidth<S>,
k_kde_bandwidth_fast<B>) and the max-density point (k_kde_max) -- what rome_kde_bandwidth[_dev] / rome_kde_max[_dev] must return for
every task of every table.

Sides, none of which is the kernel:
  * mp_fg / mp_kde_density -- mpmath at lin_ref.DPS digits, headings through lin_ref._wrap, on a named subset of tasks (MP_TASKS,
                              MP_MAX_TASKS: one per table kind and launch class; N² exponentials per evaluation).
  * np_lcv / np_g / np_root / np_kde_max -- float64 NumPy, written the plain way and NOT in the kernel's order: the full N x N
                              difference matrix (circular differences through arctan2(sin, cos)), −inf on the diagonal, row-wise
                              max-shifted log-sum-exp, Brent on g.
  * the C oracle (ro.kde_bandwidths, ro.kde_max), in tests/test_kde_ref_host.py only: same author and the same golden-section loop as the
    kernel, so it is not the independent side; it ties np_lcv to the definition that reproduces the reference's stored bandwidths.

Definition restated (the comment above ro_kde_bandwidth_lcv in oracle/rome_oracle.c):
    D_ij  = x_i − x_j                      (circular: wrapped to [−π, π])
    LL(h) = Σ_i log max(Σ_{j≠i} exp(−½ D_ij²/h²), 1e-300) − N log((N−1) h √(2π))
    minm  = max(min_{i≠j} |D_ij|, 1e-6);  maxm = max(max_i y_i − min_i y_i, minm),  y_i = D_i0 (y_0 = 0 is one of them)
    h     = golden-section minimiser of f = −LL on the bracket (2 minm/(N−1), (minm+maxm)/2, 2 maxm), Numerical-Recipes form, stop when
            |x3−x0| <= tol (|x1|+|x2|); the answer is x1 if f1 < f2, else x2.
The floor 1e-300 is part of the definition: a row whose sum underflows contributes log 1e-300 and nothing to the derivative.  With
S_i = Σ_j w_ij, T_i = Σ_j w_ij D_ij²:  dLL/dh = g(h)/h³,  g(h) = Σ_i T_i/S_i − N h²  (floored rows: 0), so a root of g where it falls
from + to − is a minimum of f.
ro_kde_max: r = max x − min x, lo = min − extend·r, hi = max + extend·r, step = (hi − lo)/(G−1), X_g = lo + g·step (X_{G−1} = hi),
y_g = Σ_j exp(−½ ((X_g − x_j)/max(h, 1e-150))²), result = X_g at the FIRST g attaining the maximum.

δ, the bound on a correct double evaluation in another order: δ = max(8·dev, 64 ulp) x scale, dev = largest |np − mp| / scale on the mp
subset.  Scales:
  f        the magnitude of what f sums, max(1, Σ_i |log S_i| + N |log((N−1) h √(2π))|) -- for the CPU margin condition and for dev_f.  f
           is the difference of two sums of that size and is much smaller than either (N = 257 bimodal: |f| = 98 of 1860), so
           relative to max(1, |f|) alone a correct evaluation is NOT within 8 eps (9.5 eps measured on the mask table, 6.5 at N = 257);
           relative to the summed magnitude it is (1.2 eps).  Every margin is recorded with both scales; the condition uses the larger
           one, which is the stricter condition.  The f-clause of rule 2 keeps max(1, |f(h_dev)|, |f(h*)|), the smaller: no GPU bound is
           wider for it.
  g        max(1, N h², Σ T_i/S_i).
  density  y_max x max(1, A) x max(1, max(|lo|, |hi|)/h), A = the exponent ½((X − x_j)/h)² of the largest weight of the top value: a sum
           of positive terms is relative to itself; the exponent carries a relative rounding of its own size into its weight; and a grid
           coordinate is only defined to an ulp of max(|lo|, |hi|), which moves a weight by that over h, relatively.

Comparison rules -- every task decided, none left out (tol = the stopping rule of the task's coordinate):
  Rule 1, same iterates: value finish with tol >= 1e-2 (every Euclidean default task, circular tasks run at 1e-2).  CPU condition: every
          decision margin |f2 − f1| of np_lcv, the final pick included, >= 1000·δ_f.  GPU: |h_dev − h_np| <= 64 ulp·h_np.  This pins the
          fast path's claim that comparisons under kTieEps = 3e-5 are re-decided in double.
  Rule 2, optimum in the reference's basin: every value-finish task (rule-1 tasks too, and the fine rules of the slow kernels, N < 8 or
          N > 128).  h* = the np minimiser of f over the reference's final 1e-2 bracket (the hull of x0, x1, x2, x3: the root of g
          when g falls through 0 there, else the end with the smaller f).  GPU: |h_dev/h* − 1| <= 2·tol/(1 − 2·tol) -- answer and minimum
          both lie in a final bracket of width <= tol(|x1|+|x2|) -- or f_np(h_dev) − f_np(h*) <= 1000·δ_f: a double-precision likelihood
          cannot tell h_dev from the optimum.
  Rule 3, derivative finish: 8 <= N <= 128 with tol < 1e-2.  h* = the root of g.  CPU condition: over the reference's 1e-2 bracket
          extended as the kernel extends it, [max(x0 − w, x0/2), x3 + w], w = x3 − x0, g sampled at 201 points changes sign exactly once,
          from + to −.  GPU: |h_dev/h* − 1| <= tol, the stopping rule the caller gave.
A table that misses a CPU condition gets another seed (RESEED).  The wide table (two clusters 1e5 apart) is the one table excused from
rule 1: the fast path stages the particles as single-precision offsets from particle 0, which at offsets of 1e5 moves the data by up to
4e-3, ~1.5 % of the bandwidth -- more than any decision margin, so the iterates need not be the reference's.  Rule 2 alone decides it.
kde_max: CPU condition: the two largest distinct density values differ by >= 1000·δ_y.  GPU: the returned coordinate is the reference's
grid point within 64 ulp x max(1, |lo|, |hi|) and nearer to it than to either neighbour.

Measured on the CPU (tests/test_kde_ref_host.py -s), in units of eps = 2^-52:
  dev_f <= 1.15   dev_g <= 1.56   dev_y <= 0.04      -- every 8·dev lies below the floor, so every δ is 64 ulp = 1.42e-14 times its scale
  smallest rule-1 decision margin: 8.5e3 δ_f (8947 decisions of 1502 tasks; bound 1000)
  rule-1 decisions of the fast-path tables with margin < kTieEps = 3e-5: 101 (the double re-evaluation runs; bound 20)
  smallest kde_max top-two gap: 5.3e3 δ_y (bound 1000)
  mask tables: the circular and the Euclidean bandwidth of a coordinate differ by >= 1.8e4 times the bound applied
The host test holds every dev under 8 eps, so no table can move a bound without failing there first.
"""
import functools
import math

import mpmath as mpm
import numpy as np
from scipy.optimize import brentq

from lin_ref import DPS, EPS, _wrap

ULP64 = 64.0 * EPS
GAP_FACTOR = 1000.0
FLOOR_S, FLOOR_MINM, FLOOR_H = 1e-300, 1e-6, 1e-150
LOG_FLOOR = math.log(FLOOR_S)
CG, RG = 0.38196601125010515180, 0.61803398874989484820
TIE_EPS = 3e-5                                               # kTieEps
WRAP_EXTENT = 3.0                                            # lcv_golden_fast: extent below it -> `nowrap`
DEFAULT_TOLS = (1e-2, 1e-6)                                  # what tol = 0 selects (Euclidean, circular)
KDE_WAVES = 4                                                # kKdeWaves


def delta(scale, dev=0.0):
    return max(8.0 * dev, ULP64) * scale


# ------------------------------------------------------------------------------------------------------------ launch arithmetic
def launch_shape(N):
    """what launch_kde_bandwidth instantiates for N particles: kernel, S (slots per lane) or B (block size), nb blocks, busy lanes,
    padded points (fast path: zero-weight points at 1e18f; slow path: idle slots shadowing particle 0)"""
    if N < 8 or N > 128:
        S = 1 if N < 8 else 4 if N <= 256 else 8
        return {"kernel": "slow", "S": S, "B": None, "nb": None, "busy": min(N, 64), "pad": 64 * S - N, "cls": "slow%d" % S}
    B = 7 if N <= 70 else 10 if N <= 100 else 13
    nb = -(-N // B)
    return {"kernel": "fast", "S": 2, "B": B, "nb": nb, "busy": nb * (nb + 1) // 2, "pad": nb * B - N, "cls": "fast%d" % B}


def rules_for(N, tol, wide=False):
    """the comparison rules that decide a task"""
    if launch_shape(N)["kernel"] == "fast" and tol < 1e-2:
        return ("3",)
    return ("1", "2") if tol >= 1e-2 and not wide else ("2",)


# ------------------------------------------------------------------------------------------------------------ float64 side
class Lik:
    """the likelihood of one task: x (N,), circ; keeps the squared difference matrix"""

    def __init__(self, x, circ):
        self.x = np.asarray(x, dtype=np.float64)
        self.circ = bool(circ)
        self.N = len(self.x)
        d = self.x[:, None] - self.x[None, :]
        if self.circ:
            d = np.arctan2(np.sin(d), np.cos(d))
        self.d = d
        self.D2 = d * d
        self.off = ~np.eye(self.N, dtype=bool)

    def _rows(self, h):
        e = -0.5 * self.D2 / (h * h)
        e[~self.off] = -np.inf
        mx = e.max(axis=1)
        w = np.exp(e - mx[:, None])
        S = w.sum(axis=1)
        return mx + np.log(S), w, S

    def fs(self, h):
        """(f, the magnitude of what f sums: Σ_i |log S_i| + N |log((N−1) h √(2π))|)"""
        lse = np.maximum(self._rows(h)[0], LOG_FLOOR)
        c = self.N * math.log((self.N - 1) * h * math.sqrt(2.0 * math.pi))
        return -(float(lse.sum()) - c), max(1.0, float(np.abs(lse).sum()) + abs(c))

    def f(self, h):
        return self.fs(h)[0]

    def g_parts(self, h):
        lse, w, S = self._rows(h)
        ts = np.where(lse > LOG_FLOOR, (w * self.D2).sum(axis=1) / S, 0.0)
        return float(ts.sum()), self.N * h * h

    def g(self, h):
        a, b = self.g_parts(h)
        return a - b

    def bracket(self):
        minm = max(float(np.abs(self.d[self.off]).min()), FLOOR_MINM)
        y = self.d[:, 0]                                                           # y_0 = 0 is among them
        maxm = max(float(y.max() - y.min()), minm)
        return minm, maxm

    def extent(self):
        y = self.d[:, 0]
        return float(y.max() - y.min())


def np_lcv(x, circ, tol, lik=None, flip=None):
    """(flip: the index of one decision to take the other way -- the host test plants a wrong tie decision with it)
    -> dict h, x0, x1, x2, x3 (final), margins [(|f2 − f1|, max(1, |f1|, |f2|), term scale) per decision, the final pick last], evals"""
    L = lik or Lik(x, circ)
    N = L.N
    minm, maxm = L.bracket()
    ax, bx, cx = 2.0 * minm / (N - 1), 0.5 * (minm + maxm), 2.0 * maxm
    x0, x3 = ax, cx
    if abs(cx - bx) > abs(bx - ax):
        x1, x2 = bx, bx + CG * (cx - bx)
    else:
        x2, x1 = bx, bx - CG * (bx - ax)
    (f1, s1), (f2, s2) = L.fs(x1), L.fs(x2)
    ne, margins = 2, []
    while abs(x3 - x0) > tol * (abs(x1) + abs(x2)) and ne < 200:
        margins.append((abs(f2 - f1), max(1.0, abs(f1), abs(f2)), max(s1, s2)))
        if (f2 < f1) != (len(margins) - 1 == flip):
            x0, x1 = x1, x2
            x2 = RG * x1 + CG * x3
            f1, s1 = f2, s2
            f2, s2 = L.fs(x2)
        else:
            x3, x2 = x2, x1
            x1 = RG * x2 + CG * x0
            f2, s2 = f1, s1
            f1, s1 = L.fs(x1)
        ne += 1
    margins.append((abs(f2 - f1), max(1.0, abs(f1), abs(f2)), max(s1, s2)))
    return {"h": x1 if (f1 < f2) != (len(margins) - 1 == flip) else x2, "x0": x0, "x1": x1, "x2": x2, "x3": x3, "margins": margins, "evals": ne}


def np_g(x, circ, h, lik=None):
    return (lik or Lik(x, circ)).g(h)


def np_root(L, lo, hi):
    """the root of g on [lo, hi] (g(lo) > 0 > g(hi)) by Brent"""
    return float(brentq(L.g, lo, hi, xtol=1e-300, rtol=8.0 * EPS, maxiter=200))


def np_argmin(L, lo, hi):
    """the minimiser of f on [lo, hi]: the root of g when g falls through 0 there, else the end with the smaller f"""
    if hi <= lo:
        return lo
    if L.g(lo) > 0.0 > L.g(hi):
        return np_root(L, lo, hi)
    return lo if L.f(lo) <= L.f(hi) else hi


def extended_bracket(r):
    w = r["x3"] - r["x0"]
    return max(r["x0"] - w, 0.5 * r["x0"]), r["x3"] + w


def single_root(L, lo, hi, n=201):
    """g sampled at n points of [lo, hi] changes sign exactly once, from + to −"""
    s = np.sign([L.g(h) for h in np.linspace(lo, hi, n)])
    ch = np.nonzero(s[1:] != s[:-1])[0]
    return len(ch) == 1 and s[0] > 0 and s[-1] < 0 and not (s == 0).any()


def np_kde_max(x, h, G, extend=0.1):
    """-> dict grid (G,), y (G,), g (first argmax), X, gap (top two distinct values, absolute; inf if all equal), lo, hi, scale"""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = float(x.min()), float(x.max())
    r = hi - lo
    lo, hi = lo - extend * r, hi + extend * r
    step = (hi - lo) / (G - 1)
    grid = lo + np.arange(G) * step
    grid[G - 1] = hi
    hb = max(float(h), FLOOR_H)
    with np.errstate(over="ignore", under="ignore"):
        a = -0.5 / (hb * hb)
        d = grid[:, None] - x[None, :]
        y = np.exp(a * d * d).sum(axis=1)
    g = int(np.argmax(y))
    u = np.unique(y)
    with np.errstate(over="ignore"):
        A = float(-a * (d[g] * d[g]).min())                                        # the exponent of the largest weight of the top value
        scale = float(y.max()) * max(1.0, A) * max(1.0, max(abs(lo), abs(hi)) / hb)
    return {"grid": grid, "y": y, "g": g, "X": float(grid[g]), "gap": float(u[-1] - u[-2]) if len(u) > 1 else math.inf, "lo": lo, "hi": hi,
            "step": step, "scale": scale}


# ------------------------------------------------------------------------------------------------------------ mpmath side
def _f(v):
    return mpm.mpf(float(v))


def mp_fg(x, circ, h):
    """(f, Σ T_i/S_i, N h²) at the current mp precision; every unordered pair once"""
    N = len(x)
    xs = [_f(v) for v in x]
    h = _f(h)
    a = -1 / (2 * h * h)
    S = [mpm.mpf(0)] * N
    T = [mpm.mpf(0)] * N
    for i in range(N):
        for j in range(i + 1, N):
            d = xs[i] - xs[j]
            if circ:
                d = _wrap(d)
            d2 = d * d
            w = mpm.exp(a * d2)
            S[i] += w; S[j] += w
            wd = w * d2
            T[i] += wd; T[j] += wd
    fl = _f(FLOOR_S)
    ll = sum(mpm.log(max(s, fl)) for s in S) - N * mpm.log((N - 1) * h * mpm.sqrt(2 * mpm.pi))
    ts = sum(t / s for s, t in zip(S, T) if s > fl)
    return -ll, ts, N * h * h


mp_f = lambda x, circ, h: mp_fg(x, circ, h)[0]
mp_g = lambda x, circ, h: (lambda r: r[1] - r[2])(mp_fg(x, circ, h))


def mp_kde_density(x, h, grid):
    """Σ_j exp(−½ ((X − x_j)/max(h, 1e-150))²) for every X of the given (double) grid"""
    hb = max(_f(h), _f(FLOOR_H))
    a = -1 / (2 * hb * hb)
    xs = [_f(v) for v in x]
    return [sum(mpm.exp(a * (_f(X) - v) ** 2) for v in xs) for X in grid]


# ------------------------------------------------------------------------------------------------------------ tables
SHAPE_N = (2, 3, 7, 8, 9, 14, 15, 63, 64, 65, 70, 71, 100, 101, 104, 105, 128, 129, 256, 257, 512)   # 104 | 105: full blocks of 13 | one more
CIRC_N = (8, 9, 64, 70, 71, 100, 101, 128, 129, 256)
CIRC_KINDS = ("concentrated", "wrapped", "uniform")
MASK_CASES = ((1, 0b0), (2, 0b01), (6, 0b101010))             # (dim, m); each run with m and its complement within dim bits
MASK_N = (100, 130)
OUTLIER_N = (100, 128)
TOLS_FINE = (1e-5, 1e-5)
TOLS_COARSE = (1e-2, 1e-2)
# table key -> seed bump, for a table whose fixed seed missed a CPU condition (tests/test_kde_ref_host.py lists them with -s)
# kde_max tables: all three missed only the top-two gap (0.077, 0.23 and 0.0012 δ_y at bump 0; G = 2 at bumps 1 .. 7 of N = 512 too).  With
# G = 2 the two grid points sit 0.1·r outside the extreme particles, whose own weights are equal: a narrow bandwidth leaves a near-tie.
# No bandwidth table missed a condition.
RESEED = {
    ("max", "pair", 64, 2): 1,
    ("max", "pair", 3, 256): 1,
    ("max", "pair", 512, 2): 8,
}


def _key_part(p):
    return p if isinstance(p, int) else sum((i + 1) * ord(c) for i, c in enumerate(str(p)))


def _seed(key):
    return 0x4B4445 + 1009 * RESEED.get(key, 0) + sum((i + 1) * 7919 * _key_part(p) for i, p in enumerate(key))


def _wrap_np(th):
    return np.arctan2(np.sin(th), np.cos(th))


def _gauss(rng, N):
    return rng.normal(rng.uniform(-5.0, 5.0), rng.uniform(0.2, 2.0), N)


def _bimodal(rng, N):
    c = rng.uniform(-5.0, 5.0)
    return np.where(rng.random(N) < 0.4, rng.normal(c - 2.0, 0.05, N), rng.normal(c + 1.0, 0.4, N))


def _heading(rng, N):
    return _wrap_np(rng.normal(math.pi - 0.02, 0.1, N))


def _table(key, bel, mask, runs, **kw):
    t = {"key": key, "bel": np.ascontiguousarray(bel), "mask": mask, "runs": tuple(runs), "wide": False, "masks": (mask,)}
    t.update(kw)
    return t


@functools.lru_cache(maxsize=None)
def shape_table(N):
    """V = 5 Pose2-like beliefs (Gaussian, bimodal 0.4 / 0.6 with widths 0.05 / 0.4, heading across ±π), mask 0b100"""
    key = ("shape", N)
    rng = np.random.default_rng(_seed(key))
    bel = np.array([[_gauss(rng, N), _bimodal(rng, N), _heading(rng, N)] for _ in range(5)])
    return _table(key, bel, 0b100, (DEFAULT_TOLS, TOLS_FINE))


@functools.lru_cache(maxsize=None)
def circ_table(N):
    """V = 7, every coordinate circular: concentrated at ±π (σ = 0.1: the `nowrap` route), wrapped σ = 1.2, uniform on the circle.  The
    last two are drawn again until their extent about particle 0 is >= 3 rad (at N = 8 about half of the draws are), so the wrapped
    body of the fast path is what runs"""
    key = ("circ", N)
    rng = np.random.default_rng(_seed(key))

    def spread(draw):
        while True:
            x = _wrap_np(draw())
            y = _wrap_np(x - x[0])
            if y.max() - y.min() >= WRAP_EXTENT:
                return x
    bel = np.array([[_wrap_np(rng.normal(math.pi * rng.choice([-1.0, 1.0]), 0.1, N)),
                     spread(lambda: rng.normal(rng.uniform(-math.pi, math.pi), 1.2, N)),
                     spread(lambda: rng.uniform(-math.pi, math.pi, N))] for _ in range(7)])
    return _table(key, bel, 0b111, (DEFAULT_TOLS, TOLS_FINE, TOLS_COARSE))


@functools.lru_cache(maxsize=None)
def mask_table(dim, m, N):
    """V·dim = 6 .. 18 tasks clustered at ±3.1 in every coordinate (σ 0.2 .. 0.5): a coordinate read with the wrong mask bit gets the
    other treatment's bandwidth, which differs by far more than the bound"""
    key = ("mask", dim, m, N)
    rng = np.random.default_rng(_seed(key))
    V = {1: 7, 2: 7, 6: 3}[dim]
    bel = np.array([[_wrap_np(rng.normal(3.1 * rng.choice([-1.0, 1.0]), rng.uniform(0.2, 0.5), N)) for _ in range(dim)] for _ in range(V)])
    full = (1 << dim) - 1
    return _table(key, bel, m, (DEFAULT_TOLS,), masks=(m, full & ~m))


@functools.lru_cache(maxsize=None)
def outlier_table(N, first):
    """N(0, 1) with one particle at 1000 (the last one, or particle 0: then every staged offset is ~1000)"""
    key = ("outlier", N, int(first))
    rng = np.random.default_rng(_seed(key))
    bel = rng.normal(0.0, 1.0, (5, 3, N))
    bel[:, :, 0 if first else N - 1] = 1000.0
    return _table(key, bel, 0, (DEFAULT_TOLS,))


@functools.lru_cache(maxsize=None)
def wide_table(N=100):
    """two clusters σ = 1 at separation 1e5: rule 2 only (module docstring)"""
    key = ("wide", N)
    rng = np.random.default_rng(_seed(key))
    bel = rng.normal(0.0, 1.0, (5, 3, N)) + np.where(rng.random((5, 3, N)) < 0.5, 0.0, 1e5)
    return _table(key, bel, 0, (DEFAULT_TOLS,), wide=True)


@functools.lru_cache(maxsize=None)
def degenerate_table(which):
    """all particles equal (N = 50), two distinct values repeated (N = 64), N = 2 (separations down to below the 1e-6 floor)"""
    key = ("degenerate", which)
    rng = np.random.default_rng(_seed(key))
    if which == "equal":
        bel = np.ones((3, 1, 50)) * np.array([0.0, 5.0, -1e3])[:, None, None]
    elif which == "two":
        bel = np.array([[np.where(rng.random(64) < 0.5, c, c + s)] for c, s in ((0.0, 1.0), (-7.0, 0.3), (100.0, 2.5))])
        bel[:, :, 0], bel[:, :, 1] = bel.min(axis=2), bel.max(axis=2)               # both values present
    else:
        bel = np.array([[[0.0, s]] for s in (1.0, -0.37, 1e-3, 1e-9, 12.5)])
    return _table(key, bel, 0, (DEFAULT_TOLS,))


def all_tables():
    """(name, maker) of every bandwidth table, built lazily"""
    for N in SHAPE_N:
        yield "shape N=%d" % N, functools.partial(shape_table, N)
    for N in CIRC_N:
        yield "circ N=%d" % N, functools.partial(circ_table, N)
    for dim, m in MASK_CASES:
        for N in MASK_N:
            yield "mask dim=%d m=%s N=%d" % (dim, bin(m), N), functools.partial(mask_table, dim, m, N)
    for N in OUTLIER_N:
        for first in (False, True):
            yield "outlier N=%d %s" % (N, "first" if first else "last"), functools.partial(outlier_table, N, first)
    yield "wide N=100", wide_table
    for which in ("equal", "two", "n2"):
        yield "degenerate %s" % which, functools.partial(degenerate_table, which)


def family(name):
    return name.split()[0]


# mp subset: (table name, v) -> every coordinate of belief v; one per table kind and launch class
MP_TASKS = tuple(("shape N=%d" % N, 0) for N in (7, 64, 100, 128, 129, 257)) + tuple(("circ N=%d" % N, 0) for N in (64, 100, 128, 129)) + (
    ("mask dim=2 m=0b1 N=100", 0), ("outlier N=100 last", 0), ("outlier N=100 first", 0), ("wide N=100", 0), ("degenerate equal", 1),
    ("degenerate two", 1), ("degenerate n2", 1))


class Reference:
    """Everything the tests need about one bandwidth table, computed once and never modified: per (mask, run, task) the np_lcv result at
    the golden section's stopping rule, the rules that decide the task, h* and the CPU conditions"""

    def __init__(self, t):
        self.table = t
        bel = t["bel"]
        self.V, self.dim, self.N = bel.shape
        self.lik = {}
        self.runs = {}
        for mask in t["masks"]:
            for tols in t["runs"]:
                self.runs[(mask, tols)] = [self._task(v, k, (mask >> k) & 1, tols[(mask >> k) & 1]) for v in range(self.V) for k in range(self.dim)]

    def _lik(self, v, k, circ):
        if (v, k, circ) not in self.lik:
            self.lik[(v, k, circ)] = Lik(self.table["bel"][v, k], circ)
        return self.lik[(v, k, circ)]

    @functools.lru_cache(maxsize=None)
    def _task(self, v, k, circ, tol):
        L = self._lik(v, k, circ)
        rules = rules_for(self.N, tol, self.table["wide"])
        r = self._lcv(v, k, circ, max(tol, 1e-2))
        out = {"v": v, "k": k, "circ": circ, "tol": tol, "rules": rules, "lcv": r, "lik": L, "ok": True, "why": ""}
        if "1" in rules:
            out["margin"] = min(m / delta(st) for m, _, st in r["margins"])
            if out["margin"] < GAP_FACTOR:
                out["ok"], out["why"] = False, "decision margin %.1f δ" % out["margin"]
        if "2" in rules:
            out["hstar"] = self._argmin(v, k, circ)
        if "3" in rules:
            lo, hi = extended_bracket(self._lcv(v, k, circ, 1e-2))
            if self._single(v, k, circ):
                out["hstar"] = self._root(v, k, circ)
            else:
                out["ok"], out["why"], out["hstar"] = False, "g has no single + to − root on the extended bracket", math.nan
        return out

    @functools.lru_cache(maxsize=None)
    def _lcv(self, v, k, circ, tol):
        return np_lcv(None, circ, tol, self._lik(v, k, circ))

    @functools.lru_cache(maxsize=None)
    def _argmin(self, v, k, circ):
        r = self._lcv(v, k, circ, 1e-2)
        pts = (r["x0"], r["x1"], r["x2"], r["x3"])
        return np_argmin(self._lik(v, k, circ), min(pts), max(pts))

    @functools.lru_cache(maxsize=None)
    def _single(self, v, k, circ):
        return single_root(self._lik(v, k, circ), *extended_bracket(self._lcv(v, k, circ, 1e-2)))

    @functools.lru_cache(maxsize=None)
    def _root(self, v, k, circ):
        return np_root(self._lik(v, k, circ), *extended_bracket(self._lcv(v, k, circ, 1e-2)))

    def failures(self):
        """the CPU conditions this table misses: [(mask, tols, v, k, why)]"""
        return [(mask, tols, r["v"], r["k"], r["why"]) for (mask, tols), rs in self.runs.items() for r in rs if not r["ok"]]

    def check(self, mask, tols, h_dev):
        """kernel bandwidths (V, dim) of one run against every task -> (figures per rule, failures)"""
        h_dev = np.asarray(h_dev, dtype=np.float64).reshape(-1)
        fig, bad = {"1": 0.0, "2": 0.0, "3": 0.0, "2f": 0}, []
        for r, h in zip(self.runs[(mask, tols)], h_dev):
            where = (r["v"], r["k"], "circ" if r["circ"] else "euclid", r["tol"])
            if not (np.isfinite(h) and h > 0):
                bad.append(("not finite and positive", where, float(h)))
                continue
            if "1" in r["rules"]:
                e = abs(h - r["lcv"]["h"]) / r["lcv"]["h"]
                fig["1"] = max(fig["1"], e)
                if not e <= ULP64:
                    bad.append(("rule 1", where, float(h), r["lcv"]["h"], e))
            if "2" in r["rules"]:
                e = abs(h / r["hstar"] - 1.0)
                if e <= 2.0 * r["tol"] / (1.0 - 2.0 * r["tol"]):
                    fig["2"] = max(fig["2"], e)
                else:                                                             # not told from the optimum by a double likelihood
                    L = r["lik"]
                    fh, fs = L.f(float(h)), L.f(r["hstar"])
                    fig["2f"] += 1
                    if not fh - fs <= GAP_FACTOR * delta(max(1.0, abs(fh), abs(fs))):
                        bad.append(("rule 2", where, float(h), r["hstar"], e, fh - fs))
            if "3" in r["rules"]:
                e = abs(h / r["hstar"] - 1.0)
                fig["3"] = max(fig["3"], e)
                if not e <= r["tol"]:
                    bad.append(("rule 3", where, float(h), r["hstar"], e))
        return fig, bad


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(dict(all_tables())[name]())


# ------------------------------------------------------------------------------------------------------------ kde_max tables
MAX_PAIRS = tuple((64, G) for G in (2, 3, 63, 64, 65, 128, 129, 192, 193, 255, 256)) + (
    (3, 65), (3, 256), (63, 64), (63, 193), (65, 65), (65, 129), (65, 256), (512, 2), (512, 63), (512, 192))
MAX_SCALE = np.array([1.0, 0.1, 3.0])
MAX_SPECIAL = {"narrow": (65, 256), "zero": (64, 200), "offset": (65, 193)}    # h = step/4; h = 0; one coordinate offset by 1e4


@functools.lru_cache(maxsize=None)
def max_table(kind, N, G):
    """("pair": V = 16, dim 3 -> 48 tasks; special tables: V = 5 -> 15 tasks, the last block has idle waves) -> bel, bw, G"""
    key = ("max", kind, N, G)
    rng = np.random.default_rng(_seed(key))
    V = 16 if kind == "pair" else 5
    bel = rng.normal(size=(V, 3, N)) * MAX_SCALE[None, :, None] + np.array([5.0, -2.0, 1e4 if kind == "offset" else 0.0])[None, :, None]
    bw = rng.uniform(0.05, 0.5, (V, 3)) * MAX_SCALE
    if kind == "narrow":
        bw = 1.2 * (bel.max(axis=2) - bel.min(axis=2)) / (G - 1) / 4.0
    if kind == "zero":
        bw = np.zeros((V, 3))
    return {"key": key, "bel": np.ascontiguousarray(bel), "bw": np.ascontiguousarray(bw), "G": G}


def all_max_tables():
    for N, G in MAX_PAIRS:
        yield "max N=%d G=%d" % (N, G), functools.partial(max_table, "pair", N, G)
    for kind, (N, G) in MAX_SPECIAL.items():
        yield "max %s N=%d G=%d" % (kind, N, G), functools.partial(max_table, kind, N, G)


MP_MAX_TASKS = (("max N=64 G=65", 0), ("max N=63 G=64", 0), ("max narrow N=65 G=256", 0), ("max offset N=65 G=193", 0))


class MaxReference:
    def __init__(self, t):
        self.table = t
        V, dim, _ = t["bel"].shape
        self.res = [np_kde_max(t["bel"][v, k], t["bw"][v, k], t["G"]) for v in range(V) for k in range(dim)]
        self.gap = min(r["gap"] / delta(r["scale"]) if math.isfinite(r["gap"]) else math.inf for r in self.res)   # in δ_y; inf: all values equal

    def check(self, out):
        out = np.asarray(out, dtype=np.float64).reshape(-1)
        bad, worst = [], 0.0
        for i, (r, X) in enumerate(zip(self.res, out)):
            tol = ULP64 * max(1.0, abs(r["lo"]), abs(r["hi"]))
            e = abs(X - r["X"])
            worst = max(worst, e / tol)
            nb = [r["grid"][j] for j in (r["g"] - 1, r["g"] + 1) if 0 <= j < len(r["grid"])]
            if not (np.isfinite(X) and e <= tol and all(e < abs(X - n) for n in nb)):
                bad.append((i, float(X), r["X"], r["g"], e / tol))
        return worst, bad


@functools.lru_cache(maxsize=None)
def max_reference(name):
    return MaxReference(dict(all_max_tables())[name]())
