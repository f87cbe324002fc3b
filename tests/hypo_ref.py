"""References for the HYPOTHESIS rows of the wave-per-row kernel k_conv (its feature-complete instantiation): rows that carry a `multihypo`
alternative (`alt_var` / `hypo_w`), a `nullhypo` probability, or both, on Pose2Pose2, bearing-range -> landmark and Pose3Pose3 (nullhypo
only).  Built on tests/conv_ref.py (tables, noise plumbing, np_root / mp_root, class Reference and its bound rule).  Two sides, neither of
which is the kernel or the oracle's convolution code: np_* (float64, written the plain way) and mp_* (mpmath at lin_ref.DPS digits).

Selection (the contract).  Row c of a table draws from Philox4x32-10 (ro.philox, pinned on known answers in tests/test_host_logic.py)
with counter (particle i, stream lo, stream hi, tag), key (seed lo, seed hi), stream = stream_offset + c (the ROW index).
  tag 4 << 16      the multihypo draw: word 0 selects (primary iff (word + 0.5) 2^-32 < hypo_w[c]), words 1-3 are its entropy uniforms
  tag 5 << 16      the nullhypo draw: word 0 selects (null iff (word + 0.5) 2^-32 < nullhypo[c]), words 1-3 are uniforms 0-2
  tag 5 << 16 | 1  words 0-2 are uniforms 3-5 (SE(3))
A uniform is (word + 0.5) 2^-32: exact in double, so is the comparison -- the selection admits no tolerance.  A prior row (dir 2) ignores
its alt_var entry; alt_var = -1 or nullhypo = 0 draws nothing.

Roots.  Fractional FIXED side (Pose2Pose2 dir 1): per row the effective fixed block where(primary, fixed, alt) is appended to the store and
the row pointed at it; conv_ref's np_root / mp_root / bounds then apply unchanged.  Fractional TARGET side (Pose2Pose2 dir 0,
bearing-range -> landmark): solved particles are the plain roots.

Entropy particles (status 0, never solved).
  null        start ∘ exp(spreadNH · sd · (U - 1/2)): SE(2) for Pose2 (t += R(θ) e_t, θ += e_θ), additive for Point2, SE(3) on the
              rotation for Pose3 (t += R e_t, R <- R Exp(e_ω)).  sd = root of the corrected Fréchet variance of the start belief's tangent
              coordinates about particle 0 (Pose2: heading differences wrapped; Pose3: Log(R_0ᵀ R_i)), replaced by 1 when <= 1e-10;
              no entropy at N = 1.  (Heading spreads of every table stay under π/2: "about particle 0" = "about the circular mean".)
  unselected  (fractional-target rows) canonical start + spreadNH · ‖mean_xy(target) - mean_xy(alt)‖ · (U - 1/2) on EVERY coordinate,
              the Pose2 heading then wrapped to (-π, π].
  both        null first, then unselected.

Bounds (nothing comes from a GPU run).  Root particles: conv_ref.Reference's rule unchanged.  Entropy particles: the same rule,
max(8·dev, 64 ulp) x row scale, where the row scale also covers the start coordinates and the entropy half-widths (spreadNH · sd / 2,
nh_spread / 2), plus stat_rel x half-width for the statistic: stat_rel = max(8 · larger deviation from mp of two float64 evaluations
in different summation orders -- sequential one-pass moments shifted by particle 0, the kernel's form, and numpy's pairwise two-pass --,
64 ulp), measured per table and printed by tests/test_hypo_ref_host.py -s.

Measured (CPU, this file's tables; printed per table by tests/test_hypo_ref_host.py -s), worst over all N, in units of eps = 2^-52:
  root dev of the effective tables (t / r)   Pose2Pose2 1.28 / 1.41   bearing-range 2.98 / --     Pose3Pose3 1.00 / 1.54
  entropy dev (t / r)                        Pose2Pose2 1.29 / 2.04   bearing-range 1.36 / --     Pose3Pose3 0.41 / 1.24
  statistic sd (one-pass / pairwise)         Pose2Pose2 7.00 / 0.72   bearing-range 9.29 / 0.64   Pose3Pose3 6.93 / 0.66
  mean distance (sequential / pairwise)      Pose2Pose2 3.31 / 1.00   bearing-range 3.43 / 1.05
Every 8·dev lies below the floor, so every rel bound is 64 ulp = 1.42e-14.  stat_rel is the floor on every table but one: bearing-range at
N = 512, where the one-pass sd is 9.29 eps off and stat_rel = 74.3 eps = 1.65e-14.  tests/test_hypo_ref_host.py holds every dev under
8 eps and the statistic's figures under max(8, 2 sqrt(N)) eps, so a table cannot move a bound without failing there first.

Snap zone (conv_ref's rule): its share is 0 on EVERY table here (rotations of the Pose3 tables are kept small enough that neither a root nor
a null particle comes within 0.1 rad of π; asserted on the CPU), so no particle is left out of any comparison.
"""
import functools
import math

import mpmath as mpm
import numpy as np

import conv_ref as CR
from conv_ref import BR0, DIMS, P2P2, P3P3
from lin_ref import DPS, _mm, _mt, _mv, _rot2, _so3_exp, _so3_log, _wrap

SPREAD_NH = 3.0                                           # rome_opts_default / IIF spreadNH
HYPO_N = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512)
PPL_OF = {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8}      # the instantiation launch_ppl_v picks
ROW_COUNTS = (1, 3, 4, 5, 11)                             # ROME_WPB = 4: one wave, a partial / full / just-started block, three blocks
WPB = 4
N_ROWS = 11
TAG_MH, TAG_NH, TAG_NH2 = 4 << 16, 5 << 16, (5 << 16) | 1
ULP64 = CR.ULP64
ZONE_CLEAR = 0.1                                          # every rotation of a Pose3 table stays this far (rad) from π
BR1_N = (63, 65, 129, 257)


def launch_ppl(N):
    """particles per lane of the k_conv instantiation launch_ppl_v picks for N <= 512"""
    return 1 if N <= 64 else 2 if N <= 128 else 4 if N <= 256 else 8


# ------------------------------------------------------------------------------------------------------------ draws
def uniforms(seed, stream, N, tag):
    """(N, 4) float64: (word + 0.5) 2^-32 of ro.philox((i, stream lo, stream hi, tag), (seed lo, seed hi)), i = 0 .. N - 1"""
    import oracle as ro
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    lo, hi = stream & 0xFFFFFFFF, (stream >> 32) & 0xFFFFFFFF
    w = np.array([ro.philox((i, lo, hi, tag), key) for i in range(N)], dtype=np.float64).reshape(N, 4)
    return (w + 0.5) * (1.0 / 4294967296.0)


def draws(t):
    """-> primary (C, N) bool, null (C, N) bool, u_mh (C, N, 3), u_nh (C, N, 6), has_alt (C,) bool"""
    Cn, N = t["n_conv"], t["N"]
    primary, null = np.ones((Cn, N), bool), np.zeros((Cn, N), bool)
    u_mh, u_nh = np.zeros((Cn, N, 3)), np.zeros((Cn, N, 6))
    has_alt = (t["alt_var"] >= 0) & (t["rows4"][:, 1] != CR.DIR_PRIOR)
    for c in range(Cn):
        st = t["stream_offset"] + c
        if has_alt[c]:
            u = uniforms(t["seed"], st, N, TAG_MH)
            primary[c], u_mh[c] = u[:, 0] < t["hypo_w"][c], u[:, 1:]
        if t["nullhypo"][c] > 0.0:
            u = uniforms(t["seed"], st, N, TAG_NH)
            null[c], u_nh[c, :, :3] = u[:, 0] < t["nullhypo"][c], u[:, 1:]
            if t["kind"] == P3P3:
                u_nh[c, :, 3:] = uniforms(t["seed"], st, N, TAG_NH2)[:, :3]
    return primary, null, u_mh, u_nh, has_alt


# ------------------------------------------------------------------------------------------------------------ the statistic
def np_tangent(kind, blk):
    """(dt, N) start block -> (N, dt) tangent coordinates about particle 0"""
    x = np.asarray(blk, dtype=np.float64).T
    d = x - x[0]
    if kind == P2P2:
        d[:, 2] = CR._np_remainder(d[:, 2])
    elif kind == P3P3:
        q = CR.q_exp(x[:, 3:])
        d[:, 3:] = CR.q_log(CR.q_mul(CR.q_conj(q[:1]), q))
    return d


def np_sd(d):
    """numpy's pairwise two-pass corrected variance, summed over the coordinates"""
    return math.sqrt(float(d.var(axis=0, ddof=1).sum())) if len(d) > 1 else 0.0


def seq_sd(d):
    """the kernel's form: one pass, sequential sums of d and d², var_k = (Σ d² - (Σ d)² / N) / (N - 1)"""
    N, dt = d.shape
    if N < 2:
        return 0.0
    v = 0.0
    for k in range(dt):
        s = s2 = 0.0
        for x in d[:, k]:
            x = float(x); s += x; s2 += x * x
        v += max(0.0, (s2 - s * s / N) / (N - 1))
    return math.sqrt(v)


def _f(v):
    return mpm.mpf(float(v))


def mp_tangent(kind, blk):
    x = np.asarray(blk, dtype=np.float64).T
    out = []
    R0 = _so3_exp([_f(v) for v in x[0, 3:]]) if kind == P3P3 else None
    for p in x:
        nt = 3 if kind == P3P3 else 2
        d = [_f(p[k]) - _f(x[0, k]) for k in range(nt)]
        if kind == P2P2:
            d.append(_wrap(_f(p[2]) - _f(x[0, 2])))
        elif kind == P3P3:
            d += _so3_log(_mm(_mt(R0), _so3_exp([_f(v) for v in p[3:]])))
        out.append(d)
    return out


def mp_sd(d):
    """two-pass corrected variance at the current mp precision"""
    N = len(d)
    if N < 2:
        return mpm.mpf(0)
    v = mpm.mpf(0)
    for k in range(len(d[0])):
        m = sum(r[k] for r in d) / N
        v += sum((r[k] - m) ** 2 for r in d) / (N - 1)
    return mpm.sqrt(v)


def mean_distance(a, b, how):
    """‖mean_xy(a) - mean_xy(b)‖ of two blocks (d, N): "seq" sequential sums (the kernel's form), "np" numpy's pairwise mean, "mp" """
    if how == "np":
        return math.hypot(a[0].mean() - b[0].mean(), a[1].mean() - b[1].mean())
    N = a.shape[1]
    if how == "seq":
        s = [0.0] * 4
        for i in range(N):
            s[0] += float(a[0, i]); s[1] += float(a[1, i]); s[2] += float(b[0, i]); s[3] += float(b[1, i])
        dx, dy = (s[0] - s[2]) / N, (s[1] - s[3]) / N
        return math.sqrt(dx * dx + dy * dy)
    dx = sum(_f(v) for v in a[0]) / N - sum(_f(v) for v in b[0]) / N
    dy = sum(_f(v) for v in a[1]) / N - sum(_f(v) for v in b[1]) / N
    return mpm.sqrt(dx * dx + dy * dy)


# ------------------------------------------------------------------------------------------------------------ entropy, float64
def np_null_entropy(kind, start, e):
    """start (N, dt) canonical coordinates, e (N, dt) = spread · (U - 1/2) -> {"t", "th" | "q"} of start ∘ exp(e)"""
    if kind == BR0:
        return {"t": start + e}
    if kind == P2P2:
        c, s = np.cos(start[:, 2]), np.sin(start[:, 2])
        v = np.stack([c * e[:, 0] - s * e[:, 1], s * e[:, 0] + c * e[:, 1]], -1)
        return {"t": start[:, :2] + v, "th": start[:, 2] + e[:, 2]}
    q = CR.q_exp(start[:, 3:])
    return {"t": start[:, :3] + CR.q_rot(q, e[:, :3]), "q": CR.q_mul(q, CR.q_exp(e[:, 3:]))}


def np_start(kind, blk):
    """canonical start coordinates (N, dt) of a target block (dt, N): the Pose2 heading wrapped"""
    x = np.array(np.asarray(blk, dtype=np.float64).T)
    if kind == P2P2:
        x[:, 2] = CR._np_remainder(x[:, 2])
    return x


# ------------------------------------------------------------------------------------------------------------ entropy, mp
def mp_entropy(kind, start, e_null, e_mh):
    """one particle: start coordinates (float64, exact), e_null / e_mh lists of mpf or None -> group element as mp_root returns it"""
    x = [_f(v) for v in start]
    if kind == BR0:
        el = [x[0], x[1]]
        for e in (e_null, e_mh):
            if e is not None:
                el = [el[0] + e[0], el[1] + e[1]]
        return (el,)
    if kind == P2P2:
        t, th = x[:2], _wrap(x[2])
        if e_null is not None:
            v = _mv(_rot2(th), e_null[:2])
            t, th = [t[0] + v[0], t[1] + v[1]], th + e_null[2]
        if e_mh is not None:
            t, th = [t[0] + e_mh[0], t[1] + e_mh[1]], th + e_mh[2]
        return (t, th)
    t, R = x[:3], _so3_exp(x[3:])
    if e_null is not None:
        v = _mv(R, e_null[:3])
        t, R = [t[k] + v[k] for k in range(3)], _mm(R, _so3_exp(e_null[3:]))
    return (t, R)


# ------------------------------------------------------------------------------------------------------------ the reference
class HypoReference:
    """Everything the tests need about one hypothesis table, computed once and never modified: the draws, the effective table and its
    conv_ref.Reference (roots), the statistic, the float64 and mp value of every entropy particle, the measured deviations, the bounds.
    ref["th"] of a solved particle is np_root's heading (compared as a wrapped difference); that of an entropy particle is the stored,
    canonical one."""

    def __init__(self, t):
        kind = self.kind = t["kind"]
        self.table = t
        Cn, N = t["n_conv"], t["N"]
        dt = DIMS[kind][2]
        rows = t["rows4"]
        self.primary, self.null, self.u_mh, self.u_nh, self.has_alt = draws(t)
        dr = rows[:, 1]
        self.frac_fixed = self.has_alt & (dr == 1) if kind == P2P2 else np.zeros(Cn, bool)
        self.frac_target = self.has_alt & ~self.frac_fixed
        self.unsel = self.frac_target[:, None] & ~self.primary
        self.entropy = self.null | self.unsel                                   # never solved, status 0
        # ---- the effective table: fractional-fixed rows read where(primary, fixed, alt)
        store = t["bel_fixed"]
        extra, rows_e = [], rows.copy()
        for c in np.nonzero(self.frac_fixed)[0]:
            extra.append(np.where(self.primary[c][None, :], store[rows[c, 2]], store[t["alt_var"][c]]))
            rows_e[c, 2] = len(store) + len(extra) - 1
        te = dict(t)
        te["bel_fixed"] = np.concatenate([store, np.array(extra)], 0) if extra else store
        te["rows4"] = rows_e
        te["edge_rows"] = tuple(mp_root_rows(t, self.frac_fixed))
        self.effective = te
        self.base = CR.Reference(te)
        self.xi = self.base.xi
        # ---- the statistic and the entropy particles
        tstore = t["bel_target"] if kind == BR0 else store
        self.start = np.stack([np_start(kind, tstore[rows[c, 3]]) for c in range(Cn)])       # (C, N, dt)
        self.sd = np.zeros(Cn); self.sd_used = np.zeros(Cn); self.nh = np.zeros(Cn)
        self.hw_null = np.zeros(Cn); self.hw_mh = np.zeros(Cn)
        self.stat_dev = {"sd_seq": 0.0, "sd_np": 0.0, "nh_seq": 0.0, "nh_np": 0.0}
        self.ref = {k: np.array(v) for k, v in self.base.root.items()}
        self.mp_ent = {}
        dev_t = dev_r = 0.0
        nt = self.ref["t"].shape[-1]
        self.scale_t, self.scale_r = np.ones(Cn), np.ones(Cn)
        with mpm.workdps(DPS), np.errstate(all="ignore"):
            for c in range(Cn):
                p_null = float(t["nullhypo"][c])
                blk = tstore[rows[c, 3]]
                sd_mp = nh_mp = None
                cur = {"t": self.start[c, :, :nt].copy()}
                if kind == P2P2:
                    cur["th"] = self.start[c, :, 2].copy()
                elif kind == P3P3:
                    cur["q"] = CR.q_exp(self.start[c, :, 3:])
                if p_null > 0.0:
                    d = np_tangent(kind, blk)
                    self.sd[c] = np_sd(d)
                    sd_mp = mp_sd(mp_tangent(kind, blk))
                    if sd_mp > mpm.mpf("1e-10"):
                        self.stat_dev["sd_seq"] = max(self.stat_dev["sd_seq"], float(abs(seq_sd(d) - sd_mp) / sd_mp))
                        self.stat_dev["sd_np"] = max(self.stat_dev["sd_np"], float(abs(self.sd[c] - sd_mp) / sd_mp))
                    else:
                        assert self.sd[c] <= 1e-10 and seq_sd(d) <= 1e-10
                        sd_mp = mpm.mpf(1)
                    self.sd_used[c] = (self.sd[c] if self.sd[c] > 1e-10 else 1.0) if N > 1 else 0.0
                    if N == 1:
                        sd_mp = mpm.mpf(0)
                    self.hw_null[c] = 0.5 * SPREAD_NH * self.sd_used[c]
                    e = SPREAD_NH * self.sd_used[c] * (self.u_nh[c, :, :dt] - 0.5)
                    moved = np_null_entropy(kind, self.start[c], e)
                    for k in cur:
                        m = self.null[c].reshape((N,) + (1,) * (cur[k].ndim - 1))
                        cur[k] = np.where(m, moved[k], cur[k])
                if self.frac_target[c]:
                    ab = tstore[t["alt_var"][c]]
                    self.nh[c] = SPREAD_NH * mean_distance(blk, ab, "np")
                    ref_mp = mean_distance(blk, ab, "mp")
                    nh_mp = SPREAD_NH * ref_mp
                    self.stat_dev["nh_seq"] = max(self.stat_dev["nh_seq"], float(abs(mean_distance(blk, ab, "seq") - ref_mp) / ref_mp))
                    self.stat_dev["nh_np"] = max(self.stat_dev["nh_np"], float(abs(self.nh[c] / SPREAD_NH - ref_mp) / ref_mp))
                    self.hw_mh[c] = 0.5 * self.nh[c]
                    e = self.nh[c] * (self.u_mh[c] - 0.5)
                    u = self.unsel[c]
                    cur["t"] = np.where(u[:, None], cur["t"] + e[:, :nt], cur["t"])
                    if kind == P2P2:
                        cur["th"] = np.where(u, cur["th"] + e[:, 2], cur["th"])
                if kind == P2P2:
                    cur["th"] = CR._np_remainder(cur["th"])
                ent = self.entropy[c]
                for k in cur:
                    m = ent.reshape((N,) + (1,) * (cur[k].ndim - 1))
                    self.ref[k][c] = np.where(m, cur[k], self.ref[k][c])
                # the row scales of the entropy particles: start coordinates, reference values, half-widths
                hw = max(self.hw_null[c], self.hw_mh[c])
                self.scale_t[c] = max(1.0, np.abs(self.start[c, :, :nt]).max(), np.abs(cur["t"]).max(), hw)
                self.scale_r[c] = max(1.0, np.abs(self.start[c, :, nt:]).max() if dt > nt else 0.0, hw)
                # mp value of every entropy particle of the row
                for i in np.nonzero(ent)[0]:
                    e_null = [SPREAD_NH * sd_mp * (_f(self.u_nh[c, i, k]) - mpm.mpf("0.5")) for k in range(dt)] if self.null[c, i] else None
                    e_mh = [nh_mp * (_f(self.u_mh[c, i, k]) - mpm.mpf("0.5")) for k in range(3)] if self.unsel[c, i] else None
                    el = mp_entropy(kind, self.start[c, i], e_null, e_mh)
                    self.mp_ent[(c, int(i))] = el
                    et, er = CR._mp_element_distance(kind, self._mine(c, i), el)
                    dev_t = max(dev_t, float(et) / self.scale_t[c]); dev_r = max(dev_r, float(er) / self.scale_r[c])
        self.dev = {"t": dev_t, "r": dev_r}
        self.rel_bound = {k: max(8.0 * v, ULP64) for k, v in self.dev.items()}
        self.stat_rel = max(8.0 * max(self.stat_dev["sd_seq"], self.stat_dev["sd_np"]), ULP64)
        self.stat_rel_mh = max(8.0 * max(self.stat_dev["nh_seq"], self.stat_dev["nh_np"]), ULP64)
        # ---- snap zone: conv_ref's membership rule applied to every reference rotation
        if kind == P3P3:
            q = self.ref["q"]
            self.to_pi = 2.0 * np.arctan2(np.abs(q[..., 0]), np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1)))
            self.zone = self.to_pi < CR.ZONE_EDGE
        else:
            self.to_pi = np.full((Cn, N), math.pi)
            self.zone = np.zeros((Cn, N), bool)
        self.zone_share = float(self.zone.mean())

    def _mine(self, c, i):
        """the float64 reference of one particle as an mp group element"""
        tt = [_f(v) for v in self.ref["t"][c, i]]
        if self.kind == BR0:
            return (tt,)
        if self.kind == P2P2:
            return (tt, _f(self.ref["th"][c, i]))
        return (tt, CR._mp_quat_matrix(self.ref["q"][c, i]))

    def bounds(self, gn_tol=0.0, n=None):
        """per-particle bounds (n, N) of the translation and the rotation part"""
        n = self.table["n_conv"] if n is None else n
        bt, br = self.base.bounds(gn_tol, n)
        ent = self.entropy[:n]
        stat = (self.stat_rel * self.hw_null + self.stat_rel_mh * self.hw_mh)[:n]
        et = self.rel_bound["t"] * self.scale_t[:n] + stat
        er = self.rel_bound["r"] * self.scale_r[:n] + stat
        return np.where(ent, et[:, None], bt[:, None]), np.where(ent, er[:, None], br[:, None])

    def expected_status(self, n=None):
        """entropy particles report 0; so does every solved particle of these tables (translations within 100, default tol)"""
        return np.zeros((self.table["n_conv"] if n is None else n, self.table["N"]), np.int32)

    def check(self, out, gn_tol=0.0, mp=False, ref=None):
        """kernel output (n, dt, N), the table's first n rows -> (figures as fractions of the bound, failures).  EVERY particle is compared
        (the snap-zone share of these tables is 0).  A particle that misses its bound but meets the value of the OTHER selection (the root
        where the reference has entropy, the start point's entropy where it has a root) is reported as a selection difference."""
        out = np.asarray(out)
        n = out.shape[0]
        assert not self.zone.any()
        bt, br = self.bounds(gn_tol, n)
        want = {k: v[:n] for k, v in (self.ref if ref is None else ref).items()}
        with np.errstate(all="ignore"):
            et, er = CR.distance(self.kind, out, want)
            ot, orr = CR.distance(self.kind, out, {k: v[:n] for k, v in self.base.root.items()})
        ok = (et <= bt) & (er <= br)
        fig = {"t": float((et / bt).max()), "r": float((er / br).max()), "entropy": int(self.entropy[:n].sum())}
        bad = []
        if not ok.all():
            miss = np.argwhere(~ok)
            swapped = [(int(c), int(i)) for c, i in miss if self.entropy[c, i] and ot[c, i] <= bt[c, i] and orr[c, i] <= br[c, i]]
            if swapped:
                bad.append(("selection differs: solved where the reference draws entropy", swapped[:4], len(swapped)))
            far = [(int(c), int(i)) for c, i in miss if not self.entropy[c, i] and max(et[c, i], er[c, i]) > 1e-6]
            if far:
                bad.append(("selection differs or wrong draw: a solved particle is nowhere near its root", far[:4], len(far)))
            bad.append(("value", miss[:4].tolist(), len(miss), fig["t"], fig["r"]))
        if mp:
            wt = wr = 0.0
            with mpm.workdps(DPS):
                for c in range(n):
                    for i in range(self.table["N"]):
                        if self.entropy[c, i]:
                            el = self.mp_ent[(c, i)]
                        elif c in self.base.mp:
                            el = self.base.mp[c][i]
                        else:
                            continue
                        mt, mr = CR.distance(self.kind, out[c, :, i], el, mp=True)
                        wt = max(wt, float(mt) / bt[c, i]); wr = max(wr, float(mr) / br[c, i])
            fig["mp_t"], fig["mp_r"] = wt, wr
            if not (wt <= 1.0 and wr <= 1.0):
                bad.append(("against mp", wt, wr))
        return fig, bad


def mp_root_rows(t, frac_fixed):
    """rows whose ROOTS the mp side serves: every fractional-fixed row (the new operand), and for N <= 129 every row"""
    if t["N"] <= 129:
        return range(t["n_conv"])
    return sorted(set(np.nonzero(frac_fixed)[0].tolist()) | {0})


def headings_in_range(th):
    """every heading in (-π, π] (as doubles: -π < θ <= π)"""
    th = np.asarray(th)
    return bool(((th > -math.pi) & (th <= math.pi)).all())


# ------------------------------------------------------------------------------------------------------------ tables
# (factor, dir, fixed, target, alt_var, hypo_w, nullhypo); the store has 9 blocks, block 4 is N copies of one particle, block 8 (the last)
# appears as an alternative; hypo_w of a row without an alternative and of the prior row is never read
KIND_OF_ROW = ("both", "alt, fixed side", "null", "plain", "w = 0", "alt, target side", "prior with an alt_var entry", "p_null = 1",
               "null, identical target", "w = 1", "both, fixed side")
ROWS = {
    P2P2: ((3, 0, 5, 2, 8, 0.6, 0.3), (0, 1, 7, 1, 3, 0.7, 0.0), (5, 1, 0, 6, -1, 0.5, 0.3), (1, 0, 8, 0, -1, 0.5, 0.0),
           (4, 0, 2, 7, 5, 0.0, 0.0), (2, 0, 6, 3, 0, 0.35, 0.0), (6, 2, 1, 5, 2, 0.5, 0.0), (0, 0, 3, 8, -1, 0.5, 1.0),
           (3, 1, 2, 4, -1, 0.5, 0.3), (5, 1, 0, 1, 6, 1.0, 0.0), (2, 1, 8, 7, 1, 0.5, 0.5)),
    # bearing-range -> landmark: the fractional side is always the target; row 6 is a second alt-only row, rows 9 / 10 are w = 1 / both
    BR0: ((3, 0, 5, 2, 8, 0.6, 0.3), (0, 0, 1, 1, 3, 0.7, 0.0), (5, 0, 0, 6, -1, 0.5, 0.3), (1, 0, 4, 0, -1, 0.5, 0.0),
          (4, 0, 2, 7, 5, 0.0, 0.0), (2, 0, 3, 3, 0, 0.35, 0.0), (6, 0, 1, 5, 2, 0.5, 0.0), (0, 0, 3, 8, -1, 0.5, 1.0),
          (3, 0, 2, 4, -1, 0.5, 0.3), (5, 0, 0, 1, 6, 1.0, 0.0), (2, 0, 5, 7, 1, 0.5, 0.5)),
    # Pose3Pose3: nullhypo only (kHypoDir = -1: the entry point refuses an alt_var column)
    P3P3: ((3, 0, 5, 2, -1, 0.5, 0.3), (0, 1, 7, 1, -1, 0.5, 0.3), (5, 1, 0, 6, -1, 0.5, 0.3), (1, 0, 8, 0, -1, 0.5, 0.0),
           (4, 0, 2, 7, -1, 0.5, 1.0), (2, 1, 6, 3, -1, 0.5, 0.0), (6, 2, 1, 5, -1, 0.5, 0.0), (0, 1, 3, 8, -1, 0.5, 1.0),
           (3, 1, 2, 4, -1, 0.5, 0.3), (5, 2, 0, 1, -1, 0.5, 0.0), (2, 0, 8, 7, -1, 0.5, 0.5)),
}
V_STORE, F_FACTORS, IDENT_BLOCK, RING_RADIUS = 9, 7, 4, 13.0


def _centres(rng):
    """block centres on a ring of 13 m: neighbours 8.9 m apart, the farthest pair 25.6 m (the means stay 5-30 m apart at every N)"""
    a = 2.0 * math.pi * np.arange(V_STORE) / V_STORE + rng.uniform(0, 1)
    return RING_RADIUS * np.stack([np.cos(a), np.sin(a)], 1)


def hypo_table(kind, N):
    """the 11-row table of one (family, N); run at the row counts ROW_COUNTS from row 0"""
    dz, df, dt, nl = DIMS[kind]
    rng = np.random.default_rng(8000 + 131 * CR.KINDS.index(kind) + N)
    spec = ROWS[kind]
    t = {"kind": kind, "N": N, "n_conv": N_ROWS, "seed": CR.SEED + 3 * N, "edge_rows": (),
         "stream_offset": (1 << 32) + 777 if N == 129 else 2000 + N,              # above 2^32 once per family
         "rows4": np.array([r[:4] for r in spec], dtype=np.int32), "alt_var": np.array([r[4] for r in spec], dtype=np.int32),
         "hypo_w": np.array([r[5] for r in spec], dtype=np.float64), "nullhypo": np.array([r[6] for r in spec], dtype=np.float64)}
    cen = _centres(rng)
    if kind == P3P3:
        t["mu"] = np.concatenate([rng.uniform(-5, 5, (F_FACTORS, 3)), CR._unit(rng, (F_FACTORS,)) * rng.uniform(0, 0.8, (F_FACTORS, 1))], 1)
        t["L"] = CR._chol_rows(rng, F_FACTORS, 6, [0.3, 0.3, 0.3, 0.02, 0.02, 0.02])
        # translation spread 0.1, rotation vectors within 0.05 of a block centre of norm <= 0.8: sd <= ~0.25, entropy angle <= 3·sd/2·√3
        c3 = np.concatenate([cen, rng.uniform(-10, 10, (V_STORE, 1))], 1)
        wc = CR._unit(rng, (V_STORE,)) * rng.uniform(0.1, 0.8, (V_STORE, 1))
        bel = np.concatenate([c3[:, :, None] + 0.1 * rng.standard_normal((V_STORE, 3, N)),
                              wc[:, :, None] + 0.03 * rng.uniform(-1, 1, (V_STORE, 3, N))], 1)
        bel[IDENT_BLOCK, 3:] *= 0.3                                             # sd falls back to 1 there: entropy angles up to 2.6
    else:
        if kind == P2P2:
            t["mu"] = rng.uniform(-5, 5, (F_FACTORS, 3)) * [1, 1, 0.6]
            t["L"] = CR._chol_rows(rng, F_FACTORS, 3, [0.3, 0.3, 0.1])
        else:
            t["mu"] = np.stack([rng.uniform(-3.1, 3.1, F_FACTORS), rng.uniform(2.0, 20.0, F_FACTORS)], 1)
            t["L"] = np.stack([rng.uniform(0.01, 0.1, F_FACTORS), rng.uniform(0.05, 0.25, F_FACTORS)], 1)
        bel = np.concatenate([cen[:, :, None] + rng.standard_normal((V_STORE, 2, N)),
                              0.3 * rng.uniform(-1, 1, (V_STORE, 1, N))], 1)     # heading spread 0.6 < π/2
        hc = rng.uniform(-math.pi, math.pi, V_STORE)
        hc[[2, 5, 7]] = (math.pi - 0.05, -math.pi + 0.1, math.pi + 0.2)         # blocks that straddle ±π (block 7: stored beyond π)
        bel[:, 2] += hc[:, None]
        keep = np.arange(V_STORE) != 7
        bel[keep, 2] = np.arctan2(np.sin(bel[keep, 2]), np.cos(bel[keep, 2]))
    bel[IDENT_BLOCK] = bel[IDENT_BLOCK][:, :1]
    t["bel_fixed"] = np.ascontiguousarray(bel)
    if kind == BR0:
        lm = _centres(rng)[:, :, None] + rng.standard_normal((V_STORE, 2, N))
        lm[IDENT_BLOCK] = lm[IDENT_BLOCK][:, :1]
        t["bel_target"] = np.ascontiguousarray(lm)
    t["mu"] = np.ascontiguousarray(t["mu"], dtype=np.float64)
    return t


def plain_table(t):
    """the same table with no hypothesis on any row (alt_var = -1, nullhypo = 0 everywhere)"""
    p = dict(t)
    p["alt_var"] = np.full_like(t["alt_var"], -1)
    p["nullhypo"] = np.zeros_like(t["nullhypo"])
    return p


@functools.lru_cache(maxsize=None)
def reference(kind, N):
    return HypoReference(hypo_table(kind, N))


# ------------------------------------------------------------------------------------------------------------ bearing-range -> pose
# A ring of roots and inflation cycles: no unique reference root, a property check.  Landmarks on the 13 m ring (neighbours 8.9 m apart),
# measured ranges 1.5-3 m with σ_ρ = 0.05: for a pose ON the ring of radius ρ_z around its own landmark the range residual against any other
# landmark is at least ‖l_a - l_b‖ - 2 ρ_z >= 8.9 - 4·σ_l - 2·3.3 > 6 σ_ρ -- the two rings of a row never intersect.
BR1_ROWS = ((3, 1, 2, 0, 5, 0.6), (0, 1, 7, 1, 3, 0.7), (5, 1, 0, 2, -1, 0.5), (1, 1, 8, 3, 4, 0.0), (4, 1, 2, 4, 6, 1.0), (2, 1, 6, 5, 8, 0.35),
            (6, 1, 1, 6, 2, 0.5))
BR1_SIGMA_L = 0.2


def br1_table(N):
    """bearing-range towards the POSE, 7 rows: fixed / alt = landmark blocks (2, N), targets = pose blocks (3, N)"""
    rng = np.random.default_rng(9100 + N)
    lm = _centres(rng)[:, :, None] + BR1_SIGMA_L * rng.uniform(-1, 1, (V_STORE, 2, N))
    poses = np.concatenate([rng.uniform(-15, 15, (len(BR1_ROWS), 2, 1)) + rng.standard_normal((len(BR1_ROWS), 2, N)),
                            rng.uniform(-math.pi, math.pi, (len(BR1_ROWS), 1, 1)) + 0.3 * rng.uniform(-1, 1, (len(BR1_ROWS), 1, N))], 1)
    return {"kind": BR0, "N": N, "n_conv": len(BR1_ROWS), "seed": CR.SEED + 5 * N, "stream_offset": 3000 + N, "edge_rows": (),
            "rows4": np.array([r[:4] for r in BR1_ROWS], dtype=np.int32), "alt_var": np.array([r[4] for r in BR1_ROWS], dtype=np.int32),
            "hypo_w": np.array([r[5] for r in BR1_ROWS], dtype=np.float64), "nullhypo": np.zeros(len(BR1_ROWS)),
            "mu": np.stack([rng.uniform(-3.1, 3.1, F_FACTORS), rng.uniform(1.5, 3.0, F_FACTORS)], 1),
            "L": np.stack([rng.uniform(0.01, 0.05, F_FACTORS), np.full(F_FACTORS, 0.05)], 1),
            "bel_fixed": np.ascontiguousarray(lm), "bel_target": np.ascontiguousarray(poses)}


def br1_landmarks(t):
    """-> primary (C, N), own (C, 2, N) = the landmark each particle's draw names, other (C, 2, N) (rows without an alternative: NaN), z"""
    primary, _, _, _, has_alt = draws(t)
    rows, lm = t["rows4"], t["bel_fixed"]
    fixed = lm[rows[:, 2]]
    alt = np.where(has_alt[:, None, None], lm[np.maximum(t["alt_var"], 0)], np.nan)
    own = np.where(primary[:, None, :], fixed, alt)
    other = np.where(primary[:, None, :], alt, fixed)
    other[~has_alt] = np.nan
    z = CR.measurements(t, CR.normals(t["seed"], t["stream_offset"], t["n_conv"], t["N"], 2))
    return primary, own, other, z


def br1_residual_mp(z, pose, l):
    """the bearing-range residual (wrapped bearing difference, range difference) of one stored pose against one landmark, mp -> floats"""
    p = ([_f(pose[0]), _f(pose[1])], _f(pose[2]))
    pl = _mv(_mt(_rot2(p[1])), [_f(l[0]) - p[0][0], _f(l[1]) - p[0][1]])
    return float(_wrap(_f(z[0]) - mpm.atan2(pl[1], pl[0]))), float(_f(z[1]) - mpm.sqrt(pl[0] * pl[0] + pl[1] * pl[1]))
