"""References for the MULTI-ROOT rows of the wave-per-row kernels (k_conv at 1, 2, 4, 8 particles per lane, lean and feature-complete, and
k_conv_big): rows whose roots form a ring or a ray, so that the start point picks the root and every solver runs
inflate_cycles x {entropy, solve}, each cycle coupled to the next through a statistic over the row's particles.  Built on
tests/conv_ref.py (noise plumbing, comparison of group elements, the bound rule of class Reference) and tests/hypo_ref.py (uniforms,
np_tangent, seq_sd, np_sd, the nullhypo contract); the mp primitives are lin_ref's.  None of it is the kernel or the oracle's convolution.

Kinds (dz, df, dt as in kFamily of rome_capi.hip, in the direction the kind names):
  br1   bearing-range -> pose        (2, 2, 3)  rome_conv_pose2point2br_dev, dir_all = 1
  p2r   Point2Point2Range            (1, 2, 2)  rome_conv_point2point2range_dev, dir 0 / dir 1 rows mixed through rows4.y (one Point2 store)
  ppr0  Pose2Point2Range -> landmark (1, 3, 2)  rome_conv_pose2point2range_dev, dir_all = 0
  ppr1  Pose2Point2Range -> pose     (1, 2, 3)  ... dir_all = 1
  pb0   Pose2Point2Bearing -> landm. (1, 3, 2)  rome_conv_pose2point2bearing_dev, dir_all = 0
  pb1   Pose2Point2Bearing -> pose   (1, 2, 3)  ... dir_all = 1

The chain of one row c (stream = stream_offset + c, the ROW index), as the header comments of rome_conv_range.hip / rome_conv_br.hpp state it:
  1. measurement  z = μ_f + σ_f ξ, ξ = ro.rng_normals(seed, stream, i, dz); σ < 0: μ - σ (erfc(-ξ/√2) - 1), Uniform(μ ± |σ|)
  2. canonical start: the target block; br1 / pb1 wrap the heading to (-π, π], ppr1 passes it through bit for bit
  3. per cycle: spread = inflation · (sd > 1e-10 ? sd : 1) when inflation > 0 and N > 1, sd = root of the summed corrected variances of
     the tangent coordinates about particle 0 of ALL N current points (a Pose2 target: the wrapped heading difference included, on ppr1
     too); entropy e = spread · (U - 1/2), U = ro.rng_entropy(seed, stream, i, cycle, dt): Point2 t += e; Pose2 t += R(θ) e_xy and
     (br1 / pb1) θ <- wrap(θ + e_θ), (ppr1) θ untouched; then the step
        range (p2r, ppr0, ppr1)  t <- a + ρ (t - a)/‖t - a‖;  t == a leaves along +x;  ρ <= 0 returns a
        pb0                      t <- a + ‖t - a‖ (cos, sin)(θ_p + b);  t == a stays
        pb1                      θ <- wrap(atan2(l - t) - b);  t == l: wrap(-b)
        br1 (ring_step)          d = l - t;  t <- l - ρ d/‖d‖;  θ <- wrap(atan2(d) - b);  t == l: t <- l - (ρ, 0), θ <- wrap(-b)
CLOSED_FORM, NEWTON and GAUSS_NEWTON share this chain; GAUSS_NEWTON returns the start of a cycle unchanged where its residual is already
within tol.  nullhypo (tag 5 << 16, hypo_ref's contract): null particles skip the cycles (they stay in the statistic with their start
value) and receive start ∘ exp(spreadNH · sd0 · (U - 1/2)) in the kind's entropy form afterwards, status 0.

Three evaluations: mp_chain (mpmath at lin_ref.DPS, float64 inputs exact, the statistic in mp, whole rows), np_chain(order="seq")
(float64, one-pass moments shifted by particle 0: the register kernels' form) and np_chain(order="pairwise") (numpy two-pass); both
float64 chains are written the plain way (np.hypot, np.arctan2, np.cos, divisions).

Comparison: conv_ref.distance's rule -- translation by its largest component, heading by the wrapped difference (a tie at ±π is not part
of it); on br1 / pb1 the stored heading must also lie in [-π, π].

Edge tables (presampled, one cycle, no inflation): every particle is an independent case, so its scale is its own and not the row's.
ρ <= 0 is part of the range kinds' contract only (the anchor, status 1 under NEWTON and GAUSS_NEWTON); br1 takes ρ > 0.  The status of
an edge case is held to the window its stored point allows: 0 where the mp residual lies below tol - 64·eps·scale, 1 above tol + that.

Bounds (nothing comes from a GPU run).  dev = the largest deviation of either np_chain order from mp_chain on the mp rows relative to the
row scale = max(1, largest |coordinate| among anchor, start, ρ, root, entropy half-width) (heading part: fixed / start headings, the
bearing, half-width).  The kernel's bound is max(8·dev, 64 ulp) x row scale, conv_ref.Reference's rule.

GAUSS_NEWTON slack.  Every step moves a point along a one-parameter curve that the accepted point shares with the root the chain names,
so a point accepted at |r| <= tol instead of being stepped lies, in exact arithmetic,
  range kinds   on the ray from a through t, at |ρ - ‖t - a‖| <= tol:                       translation tol,          heading 0
  pb0           on the circle of radius n = ‖t - a‖ about a, at angle |r| <= tol:  chord 2 n sin(tol/2) <= n·tol,     --
  pb1           at the same translation, heading off by |r| <= tol:                          translation 0,           heading tol
  br1           on the ray from l (|ρ - ‖l - t‖| <= tol) with the heading off by <= tol:    translation tol,          heading tol
of that root.  With inflation = 0 later cycles keep the curve, so the slack is added ONCE.  With inflation > 0 an acceptance before the
step of any cycle is excluded on the CPU: condition (f) holds every jittered point of a ring_table at |r| >= 1000·tol in mp, so each
cycle takes exactly the closed-form step and the slack (still added once) covers the final acceptance.
All of that holds where the functor CAN reach tol at the particle's scale, i.e. under condition (d) (64·eps·scale < tol/8: every
ring_table).  Where (d) fails (edge cases at 1e6 - 1e8) the rounding of the stored iterate alone, up to 2 ulp(scale) per coordinate, may
keep |r| above tol, and the iteration then runs all max_iters = 20 steps, each from the ROUNDED previous iterate.  A step keeps the ray
(circle) of its input, so each step may turn the ray by 2 ulp(scale)/‖t - a‖: for those particles the slack grows by
max_iters · 2 ulp(scale) in the translation and, on br1 (the heading follows the ray), max_iters · 2 ulp(scale)/ρ in the heading.  This
term is no measurement: it is the number format's spacing at the scale times the iteration count (the first version of this rule
left it out; the br1 edge at anchor 1e6, ρ = 1e-3 then missed the heading bound by 9e-9 rad under GAUSS_NEWTON only).

Conditions asserted by tests/test_ring_ref_host.py on the reference alone: (a) every jittered point keeps ‖t - a‖ >= ρ/4 (bearing kinds
and pb1: ‖t - a‖ >= 1); (b) every ρ > 0, every sd >= 1e-7; (c) every particle is compared; (d) 64·eps·scale < tol/8 on every
ring_table, the reference residual is 0: status 0 everywhere; (e) identical-start tables: sd = 0 exactly; (f) above; and every heading
difference about particle 0 stays 0.2 clear of π ("about particle 0" = "about the circular mean", no tie in the wrap of the statistic).

Measured dev (CPU; printed per table by tests/test_ring_ref_host.py -s), worst over every ring_table, in units of eps = 2^-52,
translation / heading:
  ring tables (11 and 37 rows)   br1 1.44 / 4.18   p2r 3.71 / --   ppr0 1.04 / --   ppr1 1.43 / 0 (passed through)
                                 pb0 3.99 / --     pb1 2.67 / 2.76
  edge tables (scale per case)   br1 0.65 / 1.63   range kinds 0.42 / --   pb0 0.36 / --   pb1 0.00 / 1.41
Three cycles of projection did not amplify the float64 error beyond a few eps on these tables (‖t - a‖ stays above ρ/3).  Every
8·dev lies below the floor, so every bound is the floor: 64 ulp = 1.42e-14 times the row scale (+ the GAUSS_NEWTON slack); no bound
sits above it.  The host test holds every dev under DEV_CEILING = 8 eps (the worst figure, 4.18, rounded up to a power of two), so a
table cannot move a bound without failing there first.
"""
import functools
import math

import mpmath as mpm
import numpy as np

import conv_ref as CR
import hypo_ref as HR
from lin_ref import DPS, EPS, _wrap

KINDS = ("br1", "p2r", "ppr0", "ppr1", "pb0", "pb1")
DIMS = {"br1": (2, 2, 3), "p2r": (1, 2, 2), "ppr0": (1, 3, 2), "ppr1": (1, 2, 3), "pb0": (1, 3, 2), "pb1": (1, 2, 3)}     # dz, df, dt
DIR_ALL = {"br1": 1, "p2r": 0, "ppr0": 0, "ppr1": 1, "pb0": 0, "pb1": 1}
STEP = {"br1": "ring", "p2r": "range", "ppr0": "range", "ppr1": "range", "pb0": "turn_point", "pb1": "turn_heading"}
CANONICAL = ("br1", "pb1")                   # the stored heading is wrapped
HAS_RHO = ("br1", "p2r", "ppr0", "ppr1")
RING_N = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 640)
LONG_N = (65, 513)
N_ROWS, N_LONG = HR.N_ROWS, 37
CYCLES, INFLATION, TOL = 3, 2.0, 1e-12
V_STORE, F_FACTORS = 9, 7
ULP64 = CR.ULP64
DEV_CEILING = 8.0                            # eps; see the docstring
GN_MAX_ITERS = 20                            # rome_opts_default's max_iters of GAUSS_NEWTON
GN_MARGIN = 1e3                              # condition (f): jittered residuals stay this many tol away from acceptance
WRAP_CLEAR = 0.2
ROW_UNIFORM, ROW_STRADDLE, ROW_BEYOND = 2, 5, 7
NULLHYPO = (0.3, 0.0, 0.5, 1.0, 0.0, 0.3, 0.0, 0.3, 0.0, 0.5, 0.3)


def big_chunks(N):
    """chunks of 128 particles k_conv_big walks per cycle, and the particles of the last one"""
    return -(-N // 128), N - 128 * (-(-N // 128) - 1)


def blocks(n_conv):
    return -(-n_conv // HR.WPB)


def _f(v):
    return mpm.mpf(float(v))


def _pose_target(kind):
    return DIMS[kind][2] == 3


# ------------------------------------------------------------------------------------------------------------ draws
def entropy_uniforms(seed, stream, N, cycles, dt):
    """(cycles, N, dt): ro.rng_entropy(seed, stream, i, cycle, dt)"""
    import ctypes as C
    import oracle as ro
    fn = ro.lib().ro_rng_entropy
    buf = np.zeros(dt + 3)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    out = np.empty((cycles, N, dt))
    sd, st = C.c_uint64(seed), C.c_uint64(stream)
    for cyc in range(cycles):
        for i in range(N):
            fn(sd, st, C.c_uint32(i), cyc, dt, p)
            out[cyc, i] = buf[:dt]
    return out


def measurements(t, xi):
    """z (C, N, dz) in float64"""
    f = t["rows4"][:, 0]
    dz = DIMS[t["kind"]][0]
    mu, sg = t["mu"].reshape(-1, dz)[f][:, None, :], t["L"].reshape(-1, dz)[f][:, None, :]
    erfc = np.vectorize(math.erfc, otypes=[np.float64])
    return np.where(sg >= 0.0, mu + sg * xi, mu - sg * (erfc(-xi * math.sqrt(0.5)) - 1.0))


def mp_measurement(mu, sg, xi):
    return [_f(m) + _f(s) * _f(x) if s >= 0.0 else _f(m) - _f(s) * (mpm.erfc(-_f(x) / mpm.sqrt(2)) - 1) for m, s, x in zip(mu, sg, xi)]


# ------------------------------------------------------------------------------------------------------------ float64 chain
def _np_stat(kind, cur, order, mutant):
    """sd of the current points (N, dt) about particle 0"""
    N = len(cur)
    if _pose_target(kind) and mutant == "heading_unwrapped":
        d = cur - cur[0]
    else:
        d = HR.np_tangent(CR.P2P2 if _pose_target(kind) else CR.BR0, cur.T)
    if _pose_target(kind) and mutant == "no_heading":
        d = d[:, :2]
    sd = HR.seq_sd(d) if order == "seq" else HR.np_sd(d)
    if mutant == "var_over_n":
        sd *= math.sqrt((N - 1) / N)
    return sd, (float(np.abs(d[:, 2]).max()) if d.shape[1] == 3 else 0.0)


def _np_entropy(kind, cur, e, mutant=None):
    """cur (N, dt) ∘ exp(e) in the kind's form"""
    out = cur.copy()
    if not _pose_target(kind):
        out[:, :2] += e[:, :2]
        return out
    if mutant == "world_frame":
        out[:, :2] += e[:, :2]
    else:
        c, s = np.cos(cur[:, 2]), np.sin(cur[:, 2])
        out[:, 0] += c * e[:, 0] - s * e[:, 1]
        out[:, 1] += s * e[:, 0] + c * e[:, 1]
    if kind in CANONICAL:
        out[:, 2] = CR._np_remainder(cur[:, 2] + e[:, 2])
    return out


def _np_step(kind, z, fx, cur, mutant=None):
    out = cur.copy()
    a = fx[:, :2]
    d = cur[:, :2] - a
    n = np.hypot(d[:, 0], d[:, 1])
    at = n == 0.0
    ns = np.where(at, 1.0, n)
    how = STEP[kind]
    with np.errstate(all="ignore"):
        if how == "range":
            rho = z[:, 0]
            u = np.where(at[:, None], np.array([1.0, 0.0]), d / ns[:, None])
            out[:, :2] = np.where((rho > 0.0)[:, None], a + rho[:, None] * u, a)
        elif how == "turn_point":
            ang = fx[:, 2] + z[:, 0]
            out[:, :2] = np.where(at[:, None], cur[:, :2], a + n[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1))
        elif how == "turn_heading":
            psi = np.where(at, 0.0, np.arctan2(-d[:, 1], -d[:, 0]))
            out[:, 2] = CR._np_remainder(psi + z[:, 0] if mutant == "pb1_plus_b" else psi - z[:, 0])
        else:
            rho = z[:, 1]
            u = np.where(at[:, None], np.array([1.0, 0.0]), d / ns[:, None])          # unit vector landmark -> pose
            out[:, :2] = a + rho[:, None] * np.where(at[:, None], np.array([-1.0, 0.0]), u)
            psi = np.where(at, 0.0, np.arctan2(-d[:, 1], -d[:, 0]))
            th = psi - z[:, 0]
            out[:, 2] = th if mutant == "br1_no_rewrap" else CR._np_remainder(th)
    return out


# ------------------------------------------------------------------------------------------------------------ mp chain
def _mp_stat(pose, cur):
    x0 = cur[0]
    d = [[p[0] - x0[0], p[1] - x0[1]] + ([_wrap(p[2] - x0[2])] if pose else []) for p in cur]
    return HR.mp_sd(d), max((abs(r[2]) for r in d), default=mpm.mpf(0)) if pose else mpm.mpf(0)


def _mp_entropy(kind, p, e):
    if not _pose_target(kind):
        return [p[0] + e[0], p[1] + e[1]]
    c, s = mpm.cos(p[2]), mpm.sin(p[2])
    return [p[0] + c * e[0] - s * e[1], p[1] + s * e[0] + c * e[1], _wrap(p[2] + e[2]) if kind in CANONICAL else p[2]]


def _mp_step(kind, z, fx, p):
    a = fx[:2]
    d = [p[0] - a[0], p[1] - a[1]]
    n = mpm.sqrt(d[0] * d[0] + d[1] * d[1])
    at = n == 0
    how = STEP[kind]
    if how == "range":
        if not z[0] > 0:
            return [a[0], a[1]] + p[2:]
        u = [mpm.mpf(1), mpm.mpf(0)] if at else [d[0] / n, d[1] / n]
        return [a[0] + z[0] * u[0], a[1] + z[0] * u[1]] + p[2:]
    if how == "turn_point":
        ang = fx[2] + z[0]
        return list(p) if at else [a[0] + n * mpm.cos(ang), a[1] + n * mpm.sin(ang)]
    psi = mpm.mpf(0) if at else mpm.atan2(-d[1], -d[0])
    if how == "turn_heading":
        return [p[0], p[1], _wrap(psi - z[0])]
    u = [mpm.mpf(-1), mpm.mpf(0)] if at else [d[0] / n, d[1] / n]
    return [a[0] + z[1] * u[0], a[1] + z[1] * u[1], _wrap(psi - z[0])]


def mp_residual(kind, z, fx, p):
    """largest |component| of the residual of the point p (mpf lists); the bearing is that of pl = R(θ_p)ᵀ (l - p.t), 0 where pl = 0"""
    a = fx[:2]
    d = [p[0] - a[0], p[1] - a[1]]
    n = mpm.sqrt(d[0] * d[0] + d[1] * d[1])
    how = STEP[kind]
    if how == "range":
        return abs(z[0] - n)
    if how == "turn_point":
        return abs(_wrap(z[0] - (mpm.atan2(d[1], d[0]) - fx[2]))) if n != 0 else abs(_wrap(z[0]))   # (pl = 0: atan2(0, 0) = 0, r = b)
    rb = abs(_wrap(z[0] - (mpm.atan2(-d[1], -d[0]) - p[2]))) if n != 0 else abs(_wrap(z[0]))
    return rb if how == "turn_heading" else max(rb, abs(z[1] - n))


# ------------------------------------------------------------------------------------------------------------ the reference
class RingReference:
    """One table, computed once and never modified: noise, measurements, uniforms, the two float64 chains, the mp chain of the mp rows,
    dev, the bounds and the figures of the conditions.  run(...) evaluates other (cycles, inflation) pairs, noise sources, the nullhypo
    column and the mutants of the discrimination test with the same code."""

    def __init__(self, t, mp_rows=None):
        kind = self.kind = t["kind"]
        self.table = t
        self.N, self.C = t["N"], t["n_conv"]
        dz, df, dt = DIMS[kind]
        rows = t["rows4"]
        self.presampled = "z" in t
        self.xi = None if self.presampled else CR.normals(t["seed"], t["stream_offset"], self.C, self.N, dz)
        self.z = np.asarray(t["z"], dtype=np.float64) if self.presampled else measurements(t, self.xi)        # (C, N, dz)
        tstore = t.get("bel_target", t["bel_fixed"])
        self.fx = np.swapaxes(t["bel_fixed"][rows[:, 2]], 1, 2).copy()                                       # (C, N, df)
        self.start = np.swapaxes(tstore[rows[:, 3]], 1, 2).copy()                                            # (C, N, dt)
        if kind in CANONICAL:
            self.start[..., 2] = CR._np_remainder(self.start[..., 2])
        self.cycles, self.inflation = t.get("cycles", CYCLES), t.get("inflation", INFLATION)
        self._U = {}
        self.seq = self.run("seq")
        self.pair = self.run("pairwise")
        self.ref = self.seq["out"]
        self.mp_rows = list(range(self.C)) if self.presampled else (_mp_rows_of(t) if mp_rows is None else mp_rows)
        self.mp, self.mp_fig = {}, {"min_ratio": math.inf, "min_jit_r": math.inf, "max_final_r": 0.0}
        with mpm.workdps(DPS):
            for c in self.mp_rows:
                self.mp[c] = self._mp_row(c)
        self._scales()
        self._dev()

    # ---- draws
    def uniforms(self, c, stream_row=None):
        key = c if stream_row is None else ("f", stream_row)
        if key not in self._U:
            st = self.table["stream_offset"] + (c if stream_row is None else stream_row)
            self._U[key] = entropy_uniforms(self.table["seed"], st, self.N, CYCLES, DIMS[self.kind][2])
        return self._U[key]

    def null_draw(self, c):
        p = float(self.table["nullhypo"][c])
        if p <= 0.0:
            return np.zeros(self.N, bool), np.zeros((self.N, 3))
        u = HR.uniforms(self.table["seed"], self.table["stream_offset"] + c, self.N, HR.TAG_NH)
        return u[:, 0] < p, u[:, 1:]

    # ---- float64
    def run(self, order="seq", cycles=None, inflation=None, mutant=None, z=None, nullhypo=False):
        """-> {"out" (C, N, dt), "sd" (C, cycles), "min_ratio", "max_dth", "null" (C, N)}"""
        kind, N = self.kind, self.N
        cycles = self.cycles if cycles is None else cycles
        inflation = self.inflation if inflation is None else inflation
        z = self.z if z is None else z
        dt = DIMS[kind][2]
        out = np.empty_like(self.start)
        sds = np.zeros((self.C, max(1, cycles)))
        null_all = np.zeros((self.C, N), bool)
        fig = {"min_ratio": math.inf, "max_dth": 0.0, "sd0": np.zeros(self.C)}
        ncyc = max(1, cycles) - (1 if mutant == "skip_last" and cycles > 1 else 0)
        for c in range(self.C):
            cur = self.start[c].copy()
            null, u_nh = self.null_draw(c) if nullhypo else (np.zeros(N, bool), None)
            null_all[c] = null
            sd0 = 0.0
            if nullhypo and self.table["nullhypo"][c] > 0.0 and N > 1:
                s, _ = _np_stat(kind, cur, order, None)
                sd0 = s if s > 1e-10 else 1.0
            fig["sd0"][c] = sd0
            for cyc in range(ncyc):
                jit = cur
                if inflation > 0.0 and N > 1:
                    sd, dth = _np_stat(kind, cur, order, mutant)
                    sds[c, cyc] = sd
                    fig["max_dth"] = max(fig["max_dth"], dth)
                    spread = inflation * (sd if sd > 1e-10 else 1.0)
                    U = self.uniforms(c, int(self.table["rows4"][c, 0]) if mutant == "factor_stream" else None)[cyc]
                    jit = _np_entropy(kind, cur, spread * (U - 0.5), mutant)
                new = _np_step(kind, z[c], self.fx[c], jit, mutant)
                cur = np.where(null[:, None], cur, new)
            if nullhypo and sd0 > 0.0:
                e = np.zeros((N, dt))
                e[:, :dt] = HR.SPREAD_NH * sd0 * (u_nh[:, :dt] - 0.5)
                cur = np.where(null[:, None], _np_entropy(kind, cur, e), cur)
            out[c] = cur
        return {"out": out, "sd": sds, "null": null_all, **fig}

    # ---- mp
    def _mp_row(self, c, cycles=None, inflation=None, nullhypo=False):
        kind, N, t = self.kind, self.N, self.table
        dz, df, dt = DIMS[kind]
        cycles = self.cycles if cycles is None else cycles
        inflation = self.inflation if inflation is None else inflation
        f = int(t["rows4"][c, 0])
        if self.presampled:
            z = [[_f(v) for v in self.z[c, i]] for i in range(N)]
        else:
            mu, sg = t["mu"].reshape(-1, dz)[f], t["L"].reshape(-1, dz)[f]
            z = [mp_measurement(mu, sg, self.xi[c, i]) for i in range(N)]
        fx = [[_f(v) for v in self.fx[c, i]] for i in range(N)]
        cur = [[_f(v) for v in self.start[c, i]] for i in range(N)]
        null, u_nh = self.null_draw(c) if nullhypo else (np.zeros(N, bool), None)
        sd0 = mpm.mpf(0)
        if nullhypo and t["nullhypo"][c] > 0.0 and N > 1:
            sd0 = _mp_stat(dt == 3, cur)[0]
            sd0 = sd0 if sd0 > mpm.mpf("1e-10") else mpm.mpf(1)
        half = mpm.mpf("0.5")
        rec = not nullhypo and cycles == self.cycles and inflation == self.inflation
        for cyc in range(max(1, cycles)):
            spread = None
            if inflation > 0.0 and N > 1:
                sd, _ = _mp_stat(dt == 3, cur)
                spread = _f(inflation) * (sd if sd > mpm.mpf("1e-10") else mpm.mpf(1))
                U = self.uniforms(c)[cyc]
            nxt = []
            for i in range(N):
                if null[i]:
                    nxt.append(cur[i]); continue
                p = cur[i]
                if spread is not None:
                    p = _mp_entropy(kind, p, [spread * (_f(U[i, k]) - half) for k in range(dt)])
                    if rec:
                        n = mpm.sqrt((p[0] - fx[i][0]) ** 2 + (p[1] - fx[i][1]) ** 2)
                        need = z[i][-1] / 4 if kind in HAS_RHO and kind != "pb1" else mpm.mpf(1)
                        self.mp_fig["min_ratio"] = min(self.mp_fig["min_ratio"], float(n / need))
                        self.mp_fig["min_jit_r"] = min(self.mp_fig["min_jit_r"], float(mp_residual(kind, z[i], fx[i], p)))
                nxt.append(_mp_step(kind, z[i], fx[i], p))
            cur = nxt
        if rec:
            for i in range(N):
                if not self.presampled:
                    self.mp_fig["max_final_r"] = max(self.mp_fig["max_final_r"], float(mp_residual(kind, z[i], fx[i], cur[i])))
        if nullhypo and sd0 > 0:
            for i in np.nonzero(null)[0]:
                cur[i] = _mp_entropy(kind, cur[i], [HR.SPREAD_NH * sd0 * (_f(u_nh[i, k]) - half) if k < 3 else 0 for k in range(dt)])
        return cur

    def variant(self, cycles=None, inflation=None, nullhypo=False):
        """another (cycles, inflation) pair or the nullhypo column on the same table, cached -> {"out", "null", "mp": {row: points}}"""
        key = (self.cycles if cycles is None else cycles, self.inflation if inflation is None else inflation, bool(nullhypo))
        if not hasattr(self, "_variants"):
            self._variants = {}
        if key not in self._variants:
            res = self.run("seq", key[0], key[1], nullhypo=nullhypo)
            with mpm.workdps(DPS):
                res["mp"] = {c: self._mp_row(c, key[0], key[1], nullhypo) for c in self.mp_rows}
                if nullhypo:                                                    # hypo_ref's entropy bound: + stat_rel x half-width on null particles
                    dev = 0.0
                    for c in np.nonzero(res["sd0"] > 0.0)[0]:
                        sd_mp = _mp_stat(DIMS[self.kind][2] == 3, [[_f(v) for v in p] for p in self.start[c]])[0]
                        if sd_mp > mpm.mpf("1e-10"):
                            for order in ("seq", "pairwise"):
                                dev = max(dev, float(abs(_np_stat(self.kind, self.start[c], order, None)[0] - sd_mp) / sd_mp))
                    res["stat_dev"] = dev
                    res["add"] = res["null"] * (max(8.0 * dev, ULP64) * 0.5 * HR.SPREAD_NH * res["sd0"])[:, None]
            self._variants[key] = res
        return self._variants[key]

    # ---- scales, dev, bounds
    def _scales(self):
        """(C, N) scales: one per row (the statistic couples its particles); per particle on an edge table (independent cases)"""
        kind = self.kind
        hw = 0.5 * self.inflation * np.where(self.seq["sd"] > 1e-10, self.seq["sd"], 1.0).max(axis=1) if self.inflation > 0 and self.N > 1 else np.zeros(self.C)
        if "nullhypo" in self.table and self.N > 1:                              # the nullhypo half-width spreadNH · sd0 / 2
            sd0 = np.array([_np_stat(kind, self.start[c], "seq", None)[0] for c in range(self.C)])
            hw = np.maximum(hw, 0.5 * HR.SPREAD_NH * np.where(sd0 > 1e-10, sd0, 1.0))
        m = (lambda a: np.abs(a).max(axis=-1)) if self.presampled else \
            (lambda a: np.broadcast_to(np.abs(a).reshape(self.C, -1).max(axis=1)[:, None], (self.C, self.N)))
        full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1, 1), (self.C, self.N))
        parts_t = [full(np.ones(self.C)), m(self.fx[..., :2]), m(self.start[..., :2]), m(self.ref[..., :2]), full(hw)]
        if kind in HAS_RHO:
            parts_t.append(m(self.z[..., -1:]))
        self.scale_t = np.maximum.reduce(parts_t)
        parts_r = [full(np.ones(self.C)), full(hw)]
        if DIMS[kind][1] == 3:
            parts_r.append(m(self.fx[..., 2:]))
        if DIMS[kind][2] == 3:
            parts_r.append(m(self.start[..., 2:]))
        if kind not in ("p2r", "ppr0", "ppr1"):
            parts_r.append(m(self.z[..., :1]))
        self.scale_r = np.maximum.reduce(parts_r)

    def _dev(self):
        dt = DIMS[self.kind][2]
        dev_t = dev_r = 0.0
        with mpm.workdps(DPS):
            for c in self.mp_rows:
                for res in (self.seq, self.pair):
                    for i in range(self.N):
                        et, er = self.mp_distance(res["out"][c, i], self.mp[c][i])
                        dev_t = max(dev_t, float(et) / self.scale_t[c, i]); dev_r = max(dev_r, float(er) / self.scale_r[c, i])
        self.dev = {"t": dev_t, "r": dev_r if dt == 3 else 0.0}
        self.rel_bound = {k: max(8.0 * v, ULP64) for k, v in self.dev.items()}

    def mp_distance(self, coords, el):
        o = [_f(v) for v in coords]
        et = max(abs(o[0] - el[0]), abs(o[1] - el[1]))
        return et, (abs(_wrap(o[2] - el[2])) if len(el) == 3 else mpm.mpf(0))

    def gn_slack(self, tol, n=None):
        """(n, N) translation and heading slack of GAUSS_NEWTON (the docstring's table and its max_iters term); 0 for tol = 0"""
        n = self.C if n is None else n
        how = STEP[self.kind]
        one = np.ones((n, self.N))
        d = self.ref[:n, :, :2] - self.fx[:n, :, :2]
        dist = np.hypot(d[..., 0], d[..., 1])
        if how == "range":
            gt, gr = tol * one, 0.0 * one
        elif how == "turn_point":
            gt, gr = tol * dist, 0.0 * one
        elif how == "turn_heading":
            gt, gr = 0.0 * one, tol * one
        else:
            gt, gr = tol * one, tol * one
        if tol > 0.0:                                                           # where condition (d) fails: max_iters steps from rounded iterates
            scale = np.maximum(self.scale_t[:n], self.scale_r[:n])
            stuck = ULP64 * scale >= tol / 8.0
            turn = GN_MAX_ITERS * 2.0 * EPS * scale
            gt = gt + np.where(stuck, turn, 0.0)
            if how == "ring":
                with np.errstate(all="ignore"):
                    gr = gr + np.where(stuck & (dist > 0.0), turn / np.where(dist > 0.0, dist, 1.0), 0.0)
        return gt, gr

    def bounds(self, gn_tol=0.0, n=None):
        n = self.C if n is None else n
        gt, gr = self.gn_slack(gn_tol, n)
        return self.rel_bound["t"] * self.scale_t[:n] + gt, self.rel_bound["r"] * self.scale_r[:n] + gr

    def check(self, out, gn_tol=0.0, ref=None, mp=None, rows=None, add=None):
        """kernel output (n, dt, N) of rows [0, n) (or of the listed rows) against the float64 chain of EVERY particle and, where given,
        against mp = {row: mp points} -> (figures as fractions of the bound, failures)"""
        out = np.swapaxes(np.asarray(out), 1, 2)
        rows = np.arange(out.shape[0]) if rows is None else np.asarray(rows)
        want = (self.ref if ref is None else ref)[rows]
        bt, br = self.bounds(gn_tol)
        bt, br = bt[rows], br[rows]
        if add is not None:                                                     # (the statistic's share of a null particle's bound)
            bt, br = bt + add[rows], br + add[rows]
        dt = DIMS[self.kind][2]
        with np.errstate(all="ignore"):
            et = np.abs(out[..., :2] - want[..., :2]).max(axis=-1)
            er = np.abs(CR._np_remainder(out[..., 2] - want[..., 2])) if dt == 3 else np.zeros_like(et)
        fig = {"t": float((et / bt).max()), "r": float((er / br).max())}
        ok = (et <= bt) & (er <= br)
        bad = []
        if not ok.all():
            bad.append(("value", np.argwhere(~ok)[:4].tolist(), int((~ok).sum()), fig["t"], fig["r"]))
        if self.kind in CANONICAL and not (np.abs(out[..., 2]) <= math.pi).all():
            bad.append(("a stored heading outside [-π, π]", np.argwhere(~(np.abs(out[..., 2]) <= math.pi))[:4].tolist()))
        if mp:
            wt = wr = 0.0
            with mpm.workdps(DPS):
                for k, c in enumerate(rows):
                    if int(c) not in mp:
                        continue
                    for i in range(self.N):
                        mt, mr = self.mp_distance(out[k, i], mp[int(c)][i])
                        wt = max(wt, float(mt) / bt[k, i])
                        wr = max(wr, float(mr) / br[k, i]) if dt == 3 else 0.0
            fig["mp_t"], fig["mp_r"] = wt, wr
            if not (wt <= 1.0 and wr <= 1.0):
                bad.append(("against mp", wt, wr))
        return fig, bad

    def status_window(self, out, tol=TOL, rows=None):
        """-> (must0, must1) (n, N) bool from the mp residual of the STORED points: status 0 is required where it is below tol - slack,
        status 1 where it is above tol + slack, slack = 64 eps x row scale (ρ <= 0 is never a root: status 1)"""
        out = np.swapaxes(np.asarray(out), 1, 2)
        rows = np.arange(out.shape[0]) if rows is None else np.asarray(rows)
        must0, must1 = np.zeros(out.shape[:2], bool), np.zeros(out.shape[:2], bool)
        with mpm.workdps(DPS):
            for k, c in enumerate(rows):
                for i in range(self.N):
                    slack = ULP64 * max(self.scale_t[c, i], self.scale_r[c, i], float(np.abs(out[k, i]).max()))
                    z = [_f(v) for v in self.z[c, i]]
                    r = float(mp_residual(self.kind, z, [_f(v) for v in self.fx[c, i]], [_f(v) for v in out[k, i]]))
                    neg = self.kind in HAS_RHO and not self.z[c, i, -1] > 0.0 and STEP[self.kind] == "range"
                    must0[k, i] = not neg and r < tol - slack
                    must1[k, i] = neg or r > tol + slack
        return must0, must1


def np_chain(ref, order="seq", **kw):
    """the float64 chain of a RingReference's table: order "seq" | "pairwise"; cycles, inflation, mutant, nullhypo as RingReference.run"""
    return ref.run(order, **kw)


def mp_chain(ref, c, **kw):
    """the mp chain of row c (a whole row: the statistic couples its particles) -> N points as mpf lists"""
    with mpm.workdps(DPS):
        return ref._mp_row(c, **kw)


def _mp_rows_of(t):
    """the special rows plus a seeded 5 % of the others (N >= 256: two rows in all)"""
    n, N = t["n_conv"], t["N"]
    rnd = [c for c in range(n) if c not in (ROW_UNIFORM, ROW_STRADDLE, ROW_BEYOND)]
    k = max(1, int(math.ceil(0.05 * len(rnd))))
    pick = [rnd[int(j)] for j in np.random.default_rng(700 + n + N).choice(len(rnd), size=k, replace=False)]
    if N >= 256:
        return sorted({(ROW_UNIFORM, ROW_STRADDLE, ROW_BEYOND)[N % 3], pick[0]})
    return sorted({ROW_UNIFORM, ROW_STRADDLE, ROW_BEYOND} | set(pick))


# ------------------------------------------------------------------------------------------------------------ tables
def _clipped(rng, shape):
    return np.clip(rng.standard_normal(shape), -3.0, 3.0)


def ring_table(kind, N, n_conv=N_ROWS, identical=False):
    """n_conv rows; factor and variable indices out of row order, the last block of each store in use, row 2 Uniform (σ < 0), row 5 with
    Pose2 headings straddling ±π, row 7 with fixed heading + bearing (br1 / pb1: the bearing) beyond the principal range.  Anchors within
    0.45 of the origin, target centres on the circle of radius 4 about it (spread 0.25, clipped at 3 σ; p2r: one store on a circle of
    radius 2, a row's blocks four or five places apart), ρ in 1.5-3 (σ_ρ = 0.05), inflation 2: every coordinate stays under 8.8
    (condition (d)) and every jittered point at least ρ/4 from its anchor (condition (a)).
    identical: every target block is N copies of its first particle (condition (e))."""
    dz, df, dt = DIMS[kind]
    rng = np.random.default_rng(12000 + 211 * KINDS.index(kind) + 7 * N + n_conv)
    c = np.arange(n_conv)
    V = V_STORE
    rows = np.stack([(5 * c + 3) % F_FACTORS, np.full_like(c, DIR_ALL[kind]), (7 * c + 2) % V, (4 * c + 8) % V], 1).astype(np.int32)
    if kind == "p2r":
        rows[:, 1] = c % 2
    t = {"kind": kind, "N": N, "n_conv": n_conv, "seed": CR.SEED + 11 * N, "rows4": rows, "cycles": CYCLES, "inflation": INFLATION,
         "stream_offset": (1 << 32) + 4321 if N == 129 else 4000 + N, "nullhypo": np.array([NULLHYPO[k % len(NULLHYPO)] for k in c])}
    # anchors near the origin, targets on a circle of radius 4 about it: every (anchor, target) pair is 3.5-4.5 apart
    anchors = rng.uniform(-0.35, 0.35, (V, 2, 1)) + 0.1 * rng.uniform(-1, 1, (V, 2, N))
    ang = 2.0 * math.pi * (np.arange(V) + rng.uniform(0, 1)) / V
    centres = 4.0 * np.stack([np.cos(ang), np.sin(ang)], 1)[:, :, None]
    targets = centres + 0.25 * _clipped(rng, (V, 2, N))
    hd = lambda: rng.uniform(-2.5, 2.5, (V, 1, 1)) + 0.3 * rng.uniform(-1, 1, (V, 1, N))
    fixed = np.concatenate([anchors, hd()], 1) if df == 3 else anchors
    target = np.concatenate([targets, hd()], 1) if dt == 3 else targets
    fs, ts = rows[ROW_STRADDLE % n_conv, 2], rows[ROW_STRADDLE % n_conv, 3]
    if df == 3:
        w = fixed[fs, 2] - fixed[fs, 2].mean() + math.pi                         # about π: deviations of both signs
        fixed[fs, 2] = np.arctan2(np.sin(w), np.cos(w))
        fixed[rows[ROW_BEYOND % n_conv, 2], 2] += 3.0 - fixed[rows[ROW_BEYOND % n_conv, 2], 2, 0]                # θ_p about 3.0, μ_b = 2.5
    if dt == 3:
        w = target[ts, 2] - target[ts, 2].mean() + math.pi
        target[ts, 2] = np.arctan2(np.sin(w), np.cos(w))
    if kind == "p2r":                  # one Point2 store on a circle of radius 2: blocks four places apart are 3.9 from each other
        a9 = 2.0 * math.pi * (np.arange(V) + rng.uniform(0, 1)) / V
        store = 2.0 * np.stack([np.cos(a9), np.sin(a9)], 1)[:, :, None] + 0.2 * _clipped(rng, (V, 2, N))
        rows[:, 3] = (rows[:, 2] + 4 + c % 2) % V
        t["bel_fixed"] = np.ascontiguousarray(store)
    else:
        t["bel_fixed"], t["bel_target"] = np.ascontiguousarray(fixed), np.ascontiguousarray(target)
    if identical:
        key = "bel_fixed" if kind == "p2r" else "bel_target"
        t[key] = np.ascontiguousarray(np.broadcast_to(t[key][:, :, :1], t[key].shape))
    mu_rho, sg_rho = rng.uniform(1.5, 3.0, F_FACTORS), np.full(F_FACTORS, 0.05)
    mu_b, sg_b = rng.uniform(-2.5, 2.5, F_FACTORS), rng.uniform(0.01, 0.05, F_FACTORS)
    fu, fb = rows[ROW_UNIFORM % n_conv, 0], rows[ROW_BEYOND % n_conv, 0]
    if kind in HAS_RHO and kind != "br1":
        sg_rho[fu] = -0.4
        t["mu"], t["L"] = mu_rho, sg_rho
    else:
        sg_b[fu] = -0.3
        mu_b[fb] = 2.5 if df == 3 else 3.1                                       # pb0: θ_p + b = 5.5; br1 / pb1: b itself crosses π
        if kind == "br1":
            t["mu"], t["L"] = np.stack([mu_b, mu_rho], 1), np.stack([sg_b, sg_rho], 1)
        else:
            t["mu"], t["L"] = mu_b, sg_b
    t["mu"], t["L"] = np.ascontiguousarray(t["mu"], dtype=np.float64), np.ascontiguousarray(t["L"], dtype=np.float64)
    return t


EDGE_N = 65
PI = math.pi
BEARINGS = (PI, -PI, math.nextafter(PI, 0.0), math.nextafter(-PI, 0.0), 0.0, 1.0)


def edge_cases(kind):
    """(z, fixed particle, target particle) per case: every particle of the edge table is an independent case"""
    dz, df, dt = DIMS[kind]
    how = STEP[kind]
    cases = []

    def add(z, a, tp, th_f=0.7, th_t=-1.1):
        fx = list(a) + ([th_f] if df == 3 else [])
        tt = list(tp) + ([th_t] if dt == 3 else [])
        cases.append((list(z), fx, tt))
    dirs = [(1.0, 0.0), (0.0, -1.0), (0.6, 0.8), (-0.8, 0.6), (math.cos(2.0), math.sin(2.0))]
    if how == "range" or how == "ring":
        Z = (lambda rho, b=0.3: [b, rho]) if how == "ring" else (lambda rho, b=0.0: [rho])
        for rho in ((4.0,) if how == "ring" else (-1.0, 0.0, 4.0)):              # (ρ <= 0 is documented for the range kinds only)
            add(Z(rho), (5.0, -2.0), (5.0, -2.0))                               # from t == a
            if how == "range":
                add(Z(rho), (5.0, -2.0), (6.5, -1.0))
        for m in (1e-150, 1e-8, 1.0, 1e8):
            for d in dirs:
                add(Z(10.0), (0.5, -0.25), (0.5 + m * d[0], -0.25 + m * d[1]))
                add(Z(10.0), (0.0, 0.0), (m * d[0], m * d[1]))
        for d in dirs:
            add(Z(1e-3), (1e6, -1e6), (1e6 + 3.0 * d[0], -1e6 + 3.0 * d[1]))
        add(Z(5.0), (1.0, 2.0), (4.0, 6.0)); add(Z(5.0), (1.0, 2.0), (-2.0, -2.0)); add(Z(2.0), (0.0, 0.0), (2.0, 0.0))   # on the ring, exactly
    if how != "range":
        for b in BEARINGS:
            for d in dirs:
                if how == "ring":
                    add([b, 3.0], (1.0, 1.0), (1.0 + 2.0 * d[0], 1.0 + 2.0 * d[1]), th_t=2.0)
                else:
                    add([b], (1.0, 1.0), (1.0 + 2.0 * d[0], 1.0 + 2.0 * d[1]), th_f=0.0 if b in (PI, -PI) else 2.9, th_t=3.0)
        if how != "ring":
            for b in (0.4, PI, -2.0):
                add([b], (5.0, -2.0), (5.0, -2.0))                              # t == p.t (pb0) / t == l (pb1)
            for m in (1e-150, 1e-8, 1.0, 1e8):
                for d in dirs:
                    add([0.7], (0.0, 0.0), (m * d[0], m * d[1]))
            for d in dirs:
                add([0.7], (1e6, -1e6), (1e6 + 3.0 * d[0], -1e6 + 3.0 * d[1]))
            add([0.0], (0.0, 0.0), (2.0, 0.0), th_f=0.0, th_t=PI)                # already a root, to the last bit (pb1: atan2(-2, -0...) = π)
    return cases


def edge_table(kind):
    """presampled measurements, one cycle, no inflation: the cases of edge_cases(kind), EDGE_N to a row (the last row padded with case 0)"""
    dz, df, dt = DIMS[kind]
    cases = edge_cases(kind)
    C_ = -(-len(cases) // EDGE_N)
    idx = np.arange(C_ * EDGE_N) % len(cases)
    pick = lambda k, d: np.array([cases[j][k] for j in idx]).reshape(C_, EDGE_N, d)
    z, fx, tt = pick(0, dz), pick(1, df), pick(2, dt)
    c = np.arange(C_)
    rows = np.stack([c[::-1], np.full_like(c, DIR_ALL[kind]), c[::-1], (c + 1) % C_], 1).astype(np.int32)
    bf, bt = np.empty((C_, df, EDGE_N)), np.empty((C_, dt, EDGE_N))
    bf[rows[:, 2]] = np.swapaxes(fx, 1, 2); bt[rows[:, 3]] = np.swapaxes(tt, 1, 2)
    t = {"kind": kind, "N": EDGE_N, "n_conv": C_, "seed": CR.SEED + 9, "stream_offset": 61, "rows4": rows, "cycles": 1, "inflation": 0.0,
         "mu": np.zeros((C_, dz)).reshape(-1) if dz == 1 else np.zeros((C_, dz)), "L": np.ones((C_, dz)).reshape(-1) if dz == 1 else np.ones((C_, dz)),
         "z": z, "n_cases": len(cases)}
    if kind == "p2r":
        t["bel_fixed"] = np.ascontiguousarray(np.concatenate([bf, bt], 0))
        rows[:, 3] += C_
    else:
        t["bel_fixed"], t["bel_target"] = bf, bt
    return t


@functools.lru_cache(maxsize=None)
def reference(kind, N, n_conv=N_ROWS):
    return RingReference(ring_table(kind, N, n_conv))


@functools.lru_cache(maxsize=None)
def edge_reference(kind):
    return RingReference(edge_table(kind))


@functools.lru_cache(maxsize=None)
def identical_reference(kind, N):
    return RingReference(ring_table(kind, N, identical=True), mp_rows=[0])
